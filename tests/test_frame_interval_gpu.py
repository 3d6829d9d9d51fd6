"""Whole pairs away from the one frame interval of the rest of the suite (support.TS = 50 ms): the per-pair API with its frame_dt
argument, and the streaming and batch drivers, which form every pair's interval from the stamps the frames are pushed with
(rebvio.cpp:183) and, by default, hand the device glue the gyroBiasCorrection matrices of that interval from the host's shadow
of W_Bg (glue_params_pre; REBVIO_HIP_GYRO_PRE=0: the device forms them). With one interval for every pair a shadow stepped with
the wrong pair's interval, or kept across a break, hands over the same bits; here no two neighbouring pairs share an interval.

Everything is compared with the CPU oracle, keyline sums in the kernels' order, word for word (a NaN is a NaN): every field of
every pair record and the keyline count that comes with it, the gyro state (Bg, W_Bg) at the end, and - through the per-pair API,
the streaming driver hands out no map - every keyline field of the last map. The oracle is given frame_dt as the reference forms
it (support.frame_dt_of), the per-pair API the same value, the drivers the stamps alone. What a case claims about its stream
(every pair tracks, the pairs behind a poisoned stamp fail, s_g^3 is a denormal) is asserted on the oracle and in numpy before
the library is looked at. Streams: 192x144, at most twelve frames, KW_TRACK. Each oracle run is computed once and shared."""
import numpy as np
import pytest

from conftest import params_for
from support import B  # noqa: F401
from support import (EUROC_T0, F32, KW_TRACK, STEPS_HEALTHY, assert_keylines_equal_nan, assert_pipeline_bit_identical, frame_dt_of, gyro_noise,
                     gyro_rotations, lib_pairs, lib_stream, oracle_pairs, rec, run_stream, same_records, set_forms, stamps_from, state_words)

pytestmark = pytest.mark.gpu

W, H, NPX = 192, 144, 192 * 144
TALLY = dict(pairs=0, ok=0, words=0)
W_BG_SET = (np.eye(3) * 3.0e7 + np.array([[0, 2e3, -1e3], [2e3, 0, 5e2], [-1e3, 5e2, 0]])).astype(F32)   # not the default 0.01 * I
BG_SET = np.array([2e-4, -1e-4, 3e-4], F32)


@pytest.fixture(scope="module", autouse=True)
def tally():
    yield
    print(f"\nframe intervals: {TALLY['pairs']} pairs compared with the oracle, {TALLY['ok']} of them with status 0, {TALLY['words']} words")


def compare(want, got, what):
    """a run of the library against a run of the oracle: records, gyro state and, where the run has one, the last map"""
    same_records(want["recs"], got["recs"], what)
    assert np.array_equal(canon(want["state"]), canon(got["state"])), (what, "gyro state", want["state"], got["state"])
    if got.get("last") is not None:
        assert_keylines_equal_nan(want["last"], got["last"], what=f"{what}: last map")
    TALLY["pairs"] += len(want["recs"])
    TALLY["ok"] += sum(int(r[-2] == 0) for r in want["recs"])
    TALLY["words"] += sum(len(r) for r in want["recs"]) + len(want["state"])


def canon(state):
    """state words with every NaN made the one quiet NaN"""
    f = state.view(np.float32).copy()
    f[np.isnan(f)] = np.float32(np.nan)
    return f.view(np.uint32)


# ---- streams -----------------------------------------------------------------------------------------------------------------
_streams = {}


def stream(sid):
    """(frames [12, 144, 192], camera) of synthetic stream sid; 0 is conftest's small_stream"""
    if sid not in _streams:
        from rebvio_amd import synth
        frames, cam = synth.render_stream(W, H, 12, stream_id=sid)
        frames = np.ascontiguousarray(frames)
        frames.setflags(write=False)
        _streams[sid] = (frames, cam)
    return _streams[sid]


# ---- operations between frames -------------------------------------------------------------------------------------------
# ops: {number of frames pushed: operation}. "flush": rebvio_hip_flush - a stream without rotations ends there (the pair across
# the flush does not exist), one with rotations goes on; nothing for the oracle and the per-pair API to do. "set": flush, then
# set_gyro_state(BG_SET, W_BG_SET) on both sides. "reset": reset_state on both sides, which ends either kind of stream.
def ends_stream(op, gyro):
    return op == "reset" or not gyro


def apply_state_op(side, op):
    if op == "set":
        side.set_gyro_state(BG_SET, W_BG_SET)
    elif op == "reset":
        side.reset_state()


# ---- the runners ---------------------------------------------------------------------------------------------------------------
_oracle = {}


def oracle_run(orc_mod, sid, stamps, R=None, ops=None, op_gyro=False, **kw):
    """frames 0 .. len(stamps) - 1 of stream sid through the oracle: dict(recs = record words + keyline count per pair, status, klm,
    state = gyro state words, last = keylines of the newest map). Cached: nothing in it is changed afterwards."""
    key = (sid, tuple(stamps), None if R is None else "R", tuple(sorted((ops or {}).items())), op_gyro, tuple(sorted(kw.items())))
    if key not in _oracle:
        frames, cam = stream(sid)
        orc = orc_mod.Oracle(params_for(orc_mod, cam, **dict(KW_TRACK, **kw)))
        orc.set_sum_order("device")
        out = dict(recs=[], status=[], klm=[])
        prev = None
        for k, t in enumerate(stamps):
            m = orc.detect_u8(frames[k], t)
            if prev is not None:
                po = orc.track_pair(prev, m, R_prior=None if R is None else R[k], frame_dt=frame_dt_of(stamps[k - 1], t))
                out["recs"].append(rec(po, m.size()))
                out["status"].append(po.status)
                out["klm"].append(po.klm_num)
            prev = m
            op = (ops or {}).get(k + 1)
            if op:
                apply_state_op(orc, op)
                if ends_stream(op, op_gyro):
                    prev = None
        out["state"] = state_words(orc.gyro_state())
        out["last"] = m.keylines()
        _oracle[key] = out
    return _oracle[key]


def pairs_run(B, sid, stamps, R=None, ops=None, op_gyro=False, **kw):
    """the per-pair API: rebvio_hip_track_pair with frame_dt_of the pair's stamps"""
    frames, cam = stream(sid)
    ctx = B.Context(params_for(B, cam, **dict(KW_TRACK, **kw)))
    dev = ctx.upload_frames(frames[:len(stamps)])
    recs, prev = [], None
    for k, t in enumerate(stamps):
        m = ctx.detect_u8_device(dev + k * NPX, t)
        if prev is not None:
            recs.append(rec(ctx.track_pair(prev, m, R_prior=None if R is None else R[k], frame_dt=frame_dt_of(stamps[k - 1], t)), m.size()))
            prev.release()
        prev = m
        op = (ops or {}).get(k + 1)
        if op:
            apply_state_op(ctx, op)
            if ends_stream(op, op_gyro):
                prev.release()
                prev = None
    out = dict(recs=recs, state=state_words(ctx.gyro_state()), last=m.keylines())
    ctx.close()
    return out


def stream_run(B, sid, stamps, R=None, ops=None, host=False, **kw):
    """the streaming driver: the frames pushed with their stamps (and R[k], through the gyro entry, when there are rotations)"""
    frames, cam = stream(sid)
    ctx = B.Context(params_for(B, cam, **dict(KW_TRACK, **kw)))
    dev = ctx.upload_frames(frames[:len(stamps)])
    recs = []
    for k, t in enumerate(stamps):
        if R is not None:
            out, n = ctx.push_frame_px_gyro_device(dev + k * NPX, B.PX_GRAY8, R[k], None, t)
        elif host:
            out, n = ctx.push_frame_u8(np.ascontiguousarray(frames[k]), t)
        else:
            out, n = ctx.push_frame_u8_device(dev + k * NPX, t)
        if out.status >= 0:
            recs.append(rec(out, n))
        op = (ops or {}).get(k + 1)
        if op:
            recs.extend(rec(o, n) for o, n in ctx.flush())
            apply_state_op(ctx, op)
    recs.extend(rec(o, n) for o, n in ctx.flush())
    out = dict(recs=recs, state=state_words(ctx.gyro_state()))
    ctx.close()
    return out


def batch_run(B, sids, stamps, restart=None, **kw):
    """one lane per stream of sids, every step pushed with the stamp of its frame. restart: the number of frames after which the
    batch is flushed (which ends every lane's stream) and every lane's gyro state is put back to what a fresh lane holds."""
    cam = stream(sids[0])[1]
    L = len(sids)
    b = B.Batch(params_for(B, cam, **dict(KW_TRACK, **kw)), L)
    devs = [b.lanes[l].upload_frames(stream(sids[l])[0][:len(stamps)]) for l in range(L)]
    fresh = [b.lanes[l].gyro_state() for l in range(L)]
    recs = [[] for _ in range(L)]

    def take(outs, ns):
        for l in range(L):
            if outs[l].status >= 0:
                recs[l].append(rec(outs[l], ns[l]))

    for k, t in enumerate(stamps):
        take(*b.push_u8_device([devs[l] + k * NPX for l in range(L)], t))
        if restart == k + 1:
            for outs, ns in b.flush():
                take(outs, ns)
            for l in range(L):
                b.lanes[l].set_gyro_state(*fresh[l])
    for outs, ns in b.flush():
        take(outs, ns)
    out = [dict(recs=recs[l], state=state_words(b.lanes[l].gyro_state())) for l in range(L)]
    b.close()
    return out


HEALTHY = stamps_from(STEPS_HEALTHY)


def healthy_oracle(orc_mod, sid=0, **more):
    """the healthy schedule on the oracle, with its precondition: every pair tracks"""
    want = oracle_run(orc_mod, sid, HEALTHY, **more)
    gate = KW_TRACK["global_min_matches_threshold"]
    assert all(s == 0 for s in want["status"]) and min(want["klm"]) >= max(gate, 1000), (sid, want["status"], want["klm"])
    return want


# ---- a. the healthy schedule ---------------------------------------------------------------------------------------------------
HEALTHY_CASES = [(pre, lm, "device") for pre in (None, "0") for lm in (None, "seq", "percall", "spec3")] + [(None, None, "host")]


@pytest.mark.parametrize("gyro_pre,lm,frames_from", HEALTHY_CASES,
                         ids=[f"pre-{'off' if pre else 'on'}-lm-{lm or 'default'}-{src}" for pre, lm, src in HEALTHY_CASES])
def test_healthy_schedule(orc_mod, B, monkeypatch, gyro_pre, lm, frames_from):
    """Eleven pairs at ten different intervals between 1 ms and 1 s, every LM kernel form, the glue's 3x3 matrices from the host's
    shadow and formed on the device; host frames in one case."""
    want = healthy_oracle(orc_mod)
    assert len(set(frame_dt_of(a, b) for a, b in zip(HEALTHY, HEALTHY[1:]))) == 10
    assert all(x != y for x, y in zip(STEPS_HEALTHY, STEPS_HEALTHY[1:]))   # no pair repeats its predecessor's interval
    set_forms(monkeypatch, lm=lm, REBVIO_HIP_GYRO_PRE=gyro_pre)
    what = f"lm {lm}, GYRO_PRE {gyro_pre}, {frames_from} frames"
    compare(want, pairs_run(B, 0, HEALTHY), f"per-pair API, {what}")
    compare(want, stream_run(B, 0, HEALTHY, host=frames_from == "host"), f"streaming driver, {what}")
    assert not np.array_equal(want["state"], state_words((np.zeros(3, F32), np.eye(3, dtype=F32) * F32(0.01))))   # the filter moved


def test_healthy_schedule_from_an_absolute_stamp(orc_mod, B, small_stream):
    """The same steps from a stamp of EuRoC's size (1.4e15 us; as a float it has a spacing of 2^27 us, the difference is taken in
    uint64): the records are those of the stream that starts at 0, through support's shared pipeline check."""
    frames, cam = small_stream
    want = healthy_oracle(orc_mod)
    recs = assert_pipeline_bit_identical(orc_mod, B, frames, cam, list(range(12)), KW_TRACK, 1000, "stamps from EUROC_T0",
                                         every_pair_tracks=True, stamps=stamps_from(STEPS_HEALTHY, EUROC_T0))
    same_records([r[:-1] for r in want["recs"]], recs, "oracle from EUROC_T0 vs oracle from 0")
    ctx = B.Context(params_for(B, cam, **KW_TRACK))
    got = [rec(o, n) for o, n in run_stream(ctx, ctx.upload_frames(frames), list(range(12)), NPX, stamps=stamps_from(STEPS_HEALTHY, EUROC_T0))]
    compare(want, dict(recs=got, state=state_words(ctx.gyro_state())), "streaming driver from EUROC_T0 (support.run_stream)")
    ctx.close()


# ---- b. a gyro stream ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gyro_pre", [None, "0"], ids=["pre-on", "pre-off"])
def test_gyro_stream_on_the_healthy_schedule(orc_mod, B, monkeypatch, gyro_pre):
    """push_frame_px_gyro_device with small per-frame rotations (support.gyro_rotations, the recipe of test_stream_gyro_gpu): the glue
    call that corrects pair k with interval k forms the prior of pair k + 1 and, pre-on, takes pair k's matrices by value."""
    R = gyro_rotations(list(range(12)), 5)
    want = healthy_oracle(orc_mod, R=R)
    plain = healthy_oracle(orc_mod)
    assert all(not np.array_equal(x, y) for x, y in zip(want["recs"], plain["recs"]))   # the rotations are live in every record
    frames, cam = stream(0)
    shared = oracle_pairs(orc_mod, cam, frames, R, stamps=HEALTHY, **KW_TRACK)       # support's three runners, given the stamps
    same_records(want["recs"], [rec(po, n) for po, n in shared], "support.oracle_pairs with stamps")
    set_forms(monkeypatch, REBVIO_HIP_GYRO_PRE=gyro_pre)
    recs, state = lib_pairs(B, cam, frames, R, stamps=HEALTHY, **KW_TRACK)
    compare(want, dict(recs=recs, state=state), f"track_pair(R_prior, frame_dt), GYRO_PRE {gyro_pre}")
    recs, state = lib_stream(B, cam, frames, R, stamps=HEALTHY, **KW_TRACK)
    compare(want, dict(recs=recs, state=state), f"gyro stream, GYRO_PRE {gyro_pre}")
    if gyro_pre is None:
        compare(want, pairs_run(B, 0, HEALTHY, R=R), "track_pair(R_prior, frame_dt) again, with the last map")


# ---- c. a batch -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch_head", [None, "compact1"])
def test_batch_lanes_on_the_healthy_schedule(orc_mod, B, monkeypatch, batch_head):
    """Three lanes on three streams, every step with the schedule's stamp (a batch forms the 3x3 matrices on the device): each lane
    is the oracle's run of its stream."""
    sids = (0, 1, 2)
    want = [healthy_oracle(orc_mod, sid) for sid in sids]
    assert not np.array_equal(want[0]["recs"][0], want[1]["recs"][0]) and not np.array_equal(want[1]["recs"][0], want[2]["recs"][0])
    set_forms(monkeypatch, batch_head=batch_head)
    for l, got in enumerate(batch_run(B, sids, HEALTHY)):
        compare(want[l], got, f"batch lane {l}, BATCH_DM_HEAD {batch_head}")


# ---- d. the shadow across a break --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gyro_pre", [None, "0"], ids=["pre-on", "pre-off"])
@pytest.mark.parametrize("entry", ["plain", "gyro"])
@pytest.mark.parametrize("frames_pushed,op", [(4, "flush"), (6, "set"), (6, "reset")], ids=["flush-after-pair-3", "set-after-pair-5", "reset-after-pair-5"])
def test_break_inside_the_healthy_schedule(orc_mod, B, monkeypatch, frames_pushed, op, entry, gyro_pre):
    """A flush, a set_gyro_state with another W_Bg, a reset_state in mid-stream. The pairs on the two sides of each break have
    different intervals, so a shadow that is not started again from the state the break leaves (or that was stepped once too
    often, or not at all, across a flush the stream survives) hands the next pair the wrong matrices. A stream without rotations
    ends at its flush; one with rotations goes on across a flush and across a set_gyro_state (module comment on ops)."""
    R = gyro_rotations(list(range(12)), 5) if entry == "gyro" else None
    ops = {frames_pushed: op}
    want = oracle_run(orc_mod, 0, HEALTHY, R=R, ops=ops, op_gyro=entry == "gyro")
    cut = ends_stream(op, entry == "gyro")
    assert len(want["recs"]) == 11 - int(cut) and all(s == 0 for s in want["status"]) and min(want["klm"]) >= 1000, (want["status"], want["klm"])
    before, after = STEPS_HEALTHY[frames_pushed - 2], STEPS_HEALTHY[frames_pushed + int(cut) - 1]
    assert before != after, (before, after)
    unbroken = healthy_oracle(orc_mod, R=R)["recs"]
    if op != "flush":    # the operation is live: the first pair behind it differs from the unbroken stream's
        k = frames_pushed - 1
        assert not np.array_equal(want["recs"][k], unbroken[k + int(cut)])
    set_forms(monkeypatch, REBVIO_HIP_GYRO_PRE=gyro_pre)
    what = f"{op} after {frames_pushed} frames, {entry} stream, GYRO_PRE {gyro_pre}"
    if gyro_pre is None:
        compare(want, pairs_run(B, 0, HEALTHY, R=R, ops=ops, op_gyro=entry == "gyro"), f"per-pair API, {what}")
    compare(want, stream_run(B, 0, HEALTHY, R=R, ops=ops), f"streaming driver, {what}")


# ---- e. poisoned streams -----------------------------------------------------------------------------------------------------
POISON = {"repeated-stamp": 0, "stamp-40ms-back": -40000, "150us": 150, "1us": 1}


@pytest.mark.parametrize("name", list(POISON))
def test_poisoned_stamp_ends_tracking_until_a_reset(orc_mod, B, name):
    """Six frames whose third step is a repeated stamp, a stamp that goes back (the unsigned difference is 1.8e13 s), 150 us or 1 us:
    W_Bg leaves that pair non-finite, the pair and every later one end with status 1 (rebvio.cpp:236, the path of
    test_pair_step_nan_path) and no entry reports an error. After reset_state three more frames at 50 ms track again. The per-pair
    API, the streaming driver and a two-lane batch (lanes on streams 0 and 1; the batch is flushed and its lanes' gyro state put
    back where the others are reset) give the oracle's records and state."""
    stamps = stamps_from((50000, 33333, POISON[name], 50000, 50000))
    assert stamps[3] - stamps[2] == POISON[name] and all(t >= 0 for t in stamps)
    stamps = stamps + stamps_from((50000, 50000), stamps[-1] + 50000)
    ops = {6: "reset"}
    want = [oracle_run(orc_mod, sid, stamps, ops=ops) for sid in (0, 1)]
    for w in want:
        assert w["status"] == [0, 0, 1, 1, 1, 0, 0] and min(w["klm"][:2] + w["klm"][5:]) >= 1000, (name, w["status"], w["klm"])
        assert np.isfinite(w["state"].view(np.float32)).all()
    broken = oracle_run(orc_mod, 0, stamps[:6])
    assert broken["status"] == [0, 0, 1, 1, 1] and not np.isfinite(broken["state"].view(np.float32)).all()
    compare(broken, pairs_run(B, 0, stamps[:6]), f"{name}: per-pair API, up to the reset")
    compare(broken, stream_run(B, 0, stamps[:6]), f"{name}: streaming driver, up to the reset")
    compare(want[0], pairs_run(B, 0, stamps, ops=ops), f"{name}: per-pair API")
    compare(want[0], stream_run(B, 0, stamps, ops=ops), f"{name}: streaming driver")
    for l, got in enumerate(batch_run(B, (0, 1), stamps, restart=6)):
        compare(want[l], got, f"{name}: batch lane {l}")


# ---- f. the denormal edge ----------------------------------------------------------------------------------------------------
# steps -> the oracle's statuses. Two short steps in a row cannot track in the reference's arithmetic, whatever the library does:
# the first leaves W_Bg near 1 / s_g = 8.7e14, whose determinant overflows fp32, so invert(W_Bg) is the zero matrix; at the
# second short step the sum invert(W_Bg) + RGBias is then diag(s_b = 1.4e-17) alone, whose determinant underflows to zero, and
# W_Bg comes out non-finite. (After a 50 ms step s_b is 9.4e-13 and the same sum inverts.) So the two short steps track with a
# 50 ms step between them, and the schedule with the two in a row stands here with the statuses the oracle gives.
DENORMAL = {"separated": ((50000, 200, 50000, 190, 50000), [0, 0, 0, 0, 0]), "in-a-row": ((50000, 200, 190, 50000), [0, 0, 1, 1])}


@pytest.mark.parametrize("gyro_pre", [None, "0"], ids=["pre-on", "pre-off"])
@pytest.mark.parametrize("name", list(DENORMAL))
def test_denormal_edge_of_the_gyro_noise(orc_mod, B, monkeypatch, name, gyro_pre):
    """Steps of 200 and 190 us: det(diag(s_g)) = s_g^3 is an fp32 denormal, and the inverse formed from it is still finite. The
    host's glue, the shadow and the device's own 3x3 inverses have to keep that denormal (and, in a row, to overflow and
    underflow where the oracle does)."""
    steps, statuses = DENORMAL[name]
    stamps = stamps_from(steps)
    p = params_for(orc_mod, stream(0)[1], **KW_TRACK)
    short = [k for k, d in enumerate(steps) if d < 1000]
    assert [steps[k] for k in short] == [200, 190]
    for k in short:
        s_g, _ = gyro_noise(p, frame_dt_of(stamps[k], stamps[k + 1]))
        det = F32(F32(s_g * s_g) * s_g)
        assert 0 < det < 2.0 ** -126, (k, s_g, det)
    want = oracle_run(orc_mod, 0, stamps)
    assert want["status"] == statuses and min(k for k, s in zip(want["klm"], statuses) if s == 0) >= 1000, (want["status"], want["klm"])
    assert np.isfinite(want["state"].view(np.float32)).all() == (statuses[-1] == 0)
    set_forms(monkeypatch, REBVIO_HIP_GYRO_PRE=gyro_pre)
    compare(want, pairs_run(B, 0, stamps), f"{name}: per-pair API, GYRO_PRE {gyro_pre}")
    compare(want, stream_run(B, 0, stamps), f"{name}: streaming driver, GYRO_PRE {gyro_pre}")
    for l, got in enumerate(batch_run(B, (0, 0), stamps)):
        compare(want, got, f"{name}: batch lane {l}, GYRO_PRE {gyro_pre}")
