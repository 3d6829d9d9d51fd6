"""Per-frame gyro rotations in the streaming and batch drivers (rebvio_hip_push_frame_px_gyro*, rebvio_hip_batch_push_px_gyro_device).
A frame is pushed with the gyro rotation over the interval from the frame before it; the reference rotates the old keylines with
it, corrected by the bias estimate, ahead of minimizeVel (rebvio.cpp:163-165) and weighs the visual rotation against it
(rebvio.cpp:186-190). The contract is bit identity with the per-pair API: the record of pair (k, k+1) equals
rebvio_hip_track_pair(map_k, map_k+1, R_gyro(k+1)), every word and the keyline count, and the gyro-bias state after a flush too.

Rotations of every case: for the pair of frames i -> j of the ping-pong order, R = (Ri.T @ Rj).T @ rodrigues(w) with the scene's
camera rotations Ri, Rj and w ~ U(-0.004, 0.004) rad per axis from PCG64(seed), drawn pair by pair; R cast to fp32. Every frame's
rotation differs from every other's, so the rotation of the wrong frame anywhere in the pipeline changes the records.
All streams run with the library's default parameters (12000 / 16000 keylines, global_min_matches_threshold 500)."""
import numpy as np
import pytest

from conftest import params_for
from support import B  # noqa: F401
from support import (TS, gyro_rotations, lib_pairs, lib_stream, oracle_pairs, rec, record_words, rodrigues, same_records, set_forms,
                     state_words)

pytestmark = pytest.mark.gpu

STREAMS = {                      # fixture, ping-pong order (base, total), the oracle's smallest klm_num over the stream's pairs
    "small": ("small_stream", (12, 16), 2321),
    "c2": ("c2_stream", (8, 13), 9726),
}


_cache = {}


def case(request, orc_mod, B, name):
    """frames in push order, rotations, and the three reference runs of a stream of STREAMS - computed once, never changed"""
    if name not in _cache:
        from rebvio_amd import synth
        fixture, (base, total), min_klm = STREAMS[name]
        frames, cam = request.getfixturevalue(fixture)
        order = synth.pingpong_indices(base, total)
        seq = np.ascontiguousarray(frames[order])
        R = gyro_rotations(order, 5)
        with_prior, without = oracle_pairs(orc_mod, cam, seq, R), oracle_pairs(orc_mod, cam, seq, None)
        # the precondition, on the oracle alone: every pair is a real tracked pair, and the prior is live in every record
        gate = params_for(orc_mod, cam).global_min_matches_threshold
        assert len(with_prior) == total - 1 and gate >= 500
        for k, ((po, _), (pn, _)) in enumerate(zip(with_prior, without)):
            assert po.status == 0 and po.klm_num >= min_klm and po.klm_num >= gate, (name, k, po.status, po.klm_num)
            assert not np.array_equal(np.array(po.R, np.float32).view(np.uint32), np.array(pn.R, np.float32).view(np.uint32)), (name, k)
        pairs, state = lib_pairs(B, cam, seq, R)
        _cache[name] = dict(cam=cam, seq=seq, order=order, R=R, oracle=[rec(po, n) for po, n in with_prior], pairs=pairs, state=state)
    return _cache[name]


# ---- 1. bit identity, three ways ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "c2"])
def test_oracle_per_pair_api_and_gyro_stream_are_bit_identical(request, orc_mod, B, name):
    c = case(request, orc_mod, B, name)
    same_records(c["oracle"], c["pairs"], f"{name}: oracle vs track_pair(R_prior)")
    got, st = lib_stream(B, c["cam"], c["seq"], c["R"])
    same_records(c["pairs"], got, f"{name}: track_pair(R_prior) vs push_frame_px_gyro_device")
    assert np.array_equal(st, c["state"]), (name, st, c["state"])
    assert np.abs(c["state"][:3].view(np.float32)).max() > 0     # the bias filter moved


# ---- 2. the pipeline's shape moves nothing (the look-ahead to frame k + 2 is what these shapes stress) --------------------------------
@pytest.mark.parametrize("env", [dict(REBVIO_HIP_LEAD="3", REBVIO_HIP_GROUP="1"), dict(REBVIO_HIP_LEAD="5", REBVIO_HIP_GROUP="4"),
                                 dict(REBVIO_HIP_LEAD="8", REBVIO_HIP_GROUP="2"), dict(REBVIO_HIP_LEAD="12", REBVIO_HIP_GROUP="6"),
                                 dict(REBVIO_HIP_GYRO_PRE="0"), dict(REBVIO_HIP_LM="seq"), dict(REBVIO_HIP_LM="spec")],
                         ids=["lead3-group1", "lead5-group4", "lead8-group2", "lead12-group6", "gyro-pre-off", "lm-seq", "lm-spec"])
def test_gyro_stream_does_not_depend_on_the_pipeline_shape(request, orc_mod, B, monkeypatch, env):
    c = case(request, orc_mod, B, "c2")
    set_forms(monkeypatch, **env)
    got, st = lib_stream(B, c["cam"], c["seq"], c["R"])
    same_records(c["pairs"], got, str(env))
    assert np.array_equal(st, c["state"])


# ---- 3. existing behaviour: no rotation, the identity, the two alternating --------------------------------------------------------
def test_null_and_identity_rotations_equal_the_existing_entry(request, B):
    from rebvio_amd import synth
    frames, cam = request.getfixturevalue("c2_stream")
    seq = np.ascontiguousarray(frames[synth.pingpong_indices(8, 13)])
    eye = np.eye(3, dtype=np.float32)
    want, st, launches = lib_stream(B, cam, seq, None, entry="u8", profile=True)
    assert len(want) == len(seq) - 1 and all(w[-2] == 0 for w in want)   # (status: the record's last word, in front of the keyline count)
    for what, R in (("NULL", [None] * len(seq)), ("identity", [eye] * len(seq)), ("alternating", [eye if k % 2 else None for k in range(len(seq))])):
        got, sg, lg = lib_stream(B, cam, seq, R, profile=True)
        same_records(want, got, what)
        assert np.array_equal(st, sg), what
        assert lg == launches and sum(lg.values()) > 4 * len(seq), (what, lg, launches)   # the same kernel launches per frame


# ---- 4. flushes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "c2"])
def test_gyro_stream_continues_across_a_flush(request, orc_mod, B, name):
    """Six frames with rotations, flush, then the rest: the pair across the flush starts from the un-rotated newest map, with
    its own rotation and the host's filter state; the concatenated records are the per-pair records."""
    c = case(request, orc_mod, B, name)
    got, st = lib_stream(B, c["cam"], c["seq"], c["R"], flush_after=(6,))
    same_records(c["pairs"], got, f"{name}: flush after six frames")
    assert np.array_equal(st, c["state"])
    if name == "small":   # flushes wherever the pipeline is shallow or full: after the first frame, two in a row, near the end
        got, st = lib_stream(B, c["cam"], c["seq"], c["R"], flush_after=(1, 2, 3, 9, 15))
        same_records(c["pairs"], got, "small: many flushes")
        assert np.array_equal(st, c["state"])


def test_rotation_after_a_flush_without_rotations_is_refused(request, B):
    from rebvio_amd import synth
    frames, cam = request.getfixturevalue("small_stream")
    seq = np.ascontiguousarray(frames[synth.pingpong_indices(12, 16)])
    npx = cam.width * cam.height
    R = gyro_rotations(synth.pingpong_indices(12, 16), 5)

    def run(second_half):
        ctx = B.Context(params_for(B, cam))
        dev = ctx.upload_frames(seq)
        recs = []
        for k in range(6):
            out, n = ctx.push_frame_u8_device(dev + k * npx, k * TS)
            if out.status >= 0:
                recs.append(rec(out, n))
        recs.extend(rec(o, n) for o, n in ctx.flush())
        second_half(ctx, dev, recs)
        recs.extend(rec(o, n) for o, n in ctx.flush())
        st = state_words(ctx.gyro_state())
        ctx.close()
        return recs, st

    def plain(ctx, dev, recs):
        for k in range(6, len(seq)):
            out, n = ctx.push_frame_u8_device(dev + k * npx, k * TS)
            if out.status >= 0:
                recs.append(rec(out, n))

    def refused_then_identity(ctx, dev, recs):
        with pytest.raises(B.HipError, match=r"error -7.*R_gyro"):
            ctx.push_frame_px_gyro_device(dev + 6 * npx, B.PX_GRAY8, R[6], None, 6 * TS)
        for k in range(6, len(seq)):   # the identity is accepted; the stream behind it may carry rotations again - here: none
            out, n = ctx.push_frame_px_gyro_device(dev + k * npx, B.PX_GRAY8, np.eye(3, dtype=np.float32), None, k * TS)
            if out.status >= 0:
                recs.append(rec(out, n))

    want, st = run(plain)
    assert len(want) == 5 + 9                        # a stream without rotations ends at its flush, as it always has
    got, sg = run(refused_then_identity)
    same_records(want, got, "identity after a rotation-free flush")
    assert np.array_equal(st, sg)


# ---- 5. the other entries ---------------------------------------------------------------------------------------------------------------
def test_host_frames_equal_device_frames(request, orc_mod, B):
    c = case(request, orc_mod, B, "small")
    got, st = lib_stream(B, c["cam"], c["seq"], c["R"], host=True)
    same_records(c["pairs"], got, "push_frame_px_gyro (host frames)")
    assert np.array_equal(st, c["state"])


def test_per_frame_mask_with_rotations_equals_masked_detect_and_track_pair(request, orc_mod, B):
    c = case(request, orc_mod, B, "small")
    cam = c["cam"]
    mask = (np.random.default_rng(3).random((cam.height, cam.width)) < 0.7).astype(np.uint8)
    want, st = lib_pairs(B, cam, c["seq"], c["R"], mask=mask)
    got, sg = lib_stream(B, cam, c["seq"], c["R"], mask=mask)
    same_records(want, got, "masked")
    assert np.array_equal(st, sg)
    assert not all(np.array_equal(x, y) for x, y in zip(want, c["pairs"]))   # the mask matters
    assert all(w[-2] == 0 for w in want) and want[-1][-1] > 1000                # ... and the masked stream still tracks


# ---- 6. a failing pair in the middle --------------------------------------------------------------------------------------------------
def test_blank_frame_inside_a_gyro_stream(request, orc_mod, B):
    """One all-grey frame: an empty map, and the pairs into and out of it fail (the oracle reports status 1 for both: no velocity
    comes out of an empty map, as in test_blank_frames_in_a_stream). The rotation pending for the pair behind a failed one is
    still applied: records and the final gyro state equal the per-pair API's with the same rotations."""
    c = case(request, orc_mod, B, "small")
    cam, R = c["cam"], c["R"]
    seq = c["seq"].copy()
    seq[7] = 128
    orc = oracle_pairs(orc_mod, cam, seq, R)
    assert orc[6][1] == 0 and [po.status for po, _ in orc] == [0] * 6 + [1, 1] + [0] * 7
    assert all(po.klm_num >= 2000 for po, _ in orc[8:])          # the pairs behind the blank frame track again
    want, st = lib_pairs(B, cam, seq, R)
    same_records([rec(po, n) for po, n in orc], want, "oracle vs track_pair(R_prior)")
    got, sg = lib_stream(B, cam, seq, R)
    same_records(want, got, "track_pair(R_prior) vs gyro stream")
    assert np.array_equal(st, sg)


def test_too_few_matches_in_every_pair_of_a_gyro_stream(request, orc_mod, B):
    """Status 2 (rebvio.cpp:247-252): with a match gate no pair of the stream can reach, every pair tracks, is matched and ends
    with status 2 - on the oracle, through track_pair(R_prior) and through the gyro stream alike, in every word."""
    c = case(request, orc_mod, B, "small")
    cam, seq, R = c["cam"], c["seq"], c["R"]
    kw = dict(global_min_matches_threshold=100000)
    orc = oracle_pairs(orc_mod, cam, seq, R, **kw)
    assert [po.status for po, _ in orc] == [2] * (len(seq) - 1) and all(po.klm_num > 1000 for po, _ in orc)
    want, st = lib_pairs(B, cam, seq, R, **kw)
    same_records([rec(po, n) for po, n in orc], want, "oracle vs track_pair(R_prior)")
    got, sg = lib_stream(B, cam, seq, R, **kw)
    same_records(want, got, "track_pair(R_prior) vs gyro stream")
    assert np.array_equal(st, sg)
    got, sg = lib_stream(B, cam, seq, R, flush_after=(5,), **kw)
    same_records(want, got, "with a flush")
    assert np.array_equal(st, sg)


def test_host_and_device_glue_agree_for_a_next_rotation(B):
    """rebvio_hip_test_glue with the next pair's gyro rotation set (rebvio_hip_test_glue_set_next): the host form and the device
    form of the glue are the same statements for any R_next, not only for the identity the per-pair API hands them. The state's
    prior rotation is transpose(exp(Bg') * transpose(R_next)), RT_next its transpose, has_next what was handed in."""
    ctx = B.Context(B.default_params(96, 128, keylines_ref=3000, keylines_max=4000))
    rng = np.random.default_rng(21)

    def words(a):
        a = np.ascontiguousarray(a, np.float32)
        w = a.view(np.uint32).copy()
        w[np.isnan(a)] = 0x7FC00000
        return w

    base = None
    for trial in range(24):
        n_new = int(rng.integers(300, 4000))
        nb = (n_new + 255) // 256
        rows = rng.standard_normal((nb, 300, 6)) * np.array([400.0, 400.0, 200.0, 500.0, 500.0, 300.0])
        Y = rng.standard_normal((nb, 300)) * 0.3
        xrv = np.zeros((nb, 32), np.float32)
        iu = np.triu_indices(6)
        for b in range(nb):
            xrv[b, :21] = (rows[b].T @ rows[b])[iu]
            xrv[b, 21:27] = rows[b].T @ Y[b]
            xrv[b, 27] = 300
        J = rng.standard_normal((200, 3)) * [300.0, 300.0, 150.0]
        JtJ = J.T @ J
        JtJ6 = np.array([JtJ[0, 0], JtJ[1, 1], JtJ[2, 2], JtJ[0, 1], JtJ[0, 2], JtJ[1, 2]], np.float32)
        vel = (rng.standard_normal(3) * 0.01).astype(np.float32)
        Bg = (rng.standard_normal(3) * [1e-5, 3e-4, 1e-2][trial % 3]).astype(np.float32)
        W_Bg = (np.eye(3) * 1e4).astype(np.float32)
        Rp = rodrigues(rng.standard_normal(3) * 0.01).astype(np.float32)
        args = (vel, JtJ6, 100.0, 1.0, 31, xrv, n_new, 0.05, Bg, W_Bg, Rp)
        ctx.test_glue_set_next(None)
        (_, s0, g0), _ = ctx.test_glue(*args)
        for has_next in (True, False):
            Rn = rodrigues(rng.standard_normal(3) * [0.004, 0.05, 0.5][trial % 3]).astype(np.float32)
            ctx.test_glue_set_next(Rn, has_next)
            (od, sd, gd), (oh, sh, gh) = ctx.test_glue(*args)
            assert np.array_equal(words(record_words(od)), words(record_words(oh))), trial
            assert np.array_equal(words(sd), words(sh)) and np.array_equal(words(gd), words(gh)), trial
            assert gh.view(np.int32)[43] == int(has_next), trial
            R_state, RT_next = sh[12:21].reshape(3, 3), gh[33:42].reshape(3, 3)
            assert np.array_equal(R_state.T.view(np.uint32), RT_next.view(np.uint32))
            want = (rodrigues(sh[:3].astype(np.float64)) @ Rn.astype(np.float64).T).T      # rebvio.cpp:163-164 with the corrected bias
            assert np.abs(R_state - want).max() < 2e-6, (trial, R_state, want)
            assert not np.array_equal(words(sd[12:21]), words(s0[12:21]))                  # the rotation is live ...
            assert np.array_equal(words(sd[:12]), words(s0[:12])) and np.array_equal(words(gd[:33]), words(g0[:33]))   # ... there only
    ctx.test_glue_set_next(None)
    ctx.close()


# ---- 7. batch ---------------------------------------------------------------------------------------------------------------------------
def test_batch_lanes_with_rotations_equal_stand_alone_contexts(B):
    from rebvio_amd import synth
    W, H, L = 192, 144, 3
    order = synth.pingpong_indices(12, 16)
    cam = synth.render_stream(W, H, 1)[1]
    seqs = [np.ascontiguousarray(synth.render_stream(W, H, 12, stream_id=l)[0][order]) for l in range(L)]
    rots = [gyro_rotations(order, 5, 0), gyro_rotations(order, 6, 1), [None] * len(order)]

    def batch(gyro):
        b = B.Batch(params_for(B, cam), L)
        devs = [b.lanes[l].upload_frames(seqs[l]) for l in range(L)]
        recs = [[] for _ in range(L)]

        def take(outs, ns):
            for l in range(L):
                if outs[l].status >= 0:
                    recs[l].append(rec(outs[l], ns[l]))

        for k in range(len(order)):
            fr = [devs[l] + k * W * H for l in range(L)]
            if gyro:
                take(*b.push_px_gyro_device(fr, B.PX_GRAY8, [rots[l][k] for l in range(L)], None, k * TS))
            else:
                take(*b.push_u8_device(fr, k * TS))
        for outs, ns in b.flush():
            take(outs, ns)
        states = [state_words(c.gyro_state()) for c in b.lanes]
        b.close()
        return recs, states

    got, states = batch(True)
    plain, _ = batch(False)
    for l in range(L):
        want, st = lib_stream(B, cam, seqs[l], rots[l])
        same_records(want, got[l], f"lane {l} vs a stand-alone context")
        assert np.array_equal(st, states[l]), l
        assert len(want) == len(order) - 1 and all(w[-2] == 0 for w in want), l
    same_records(plain[2], got[2], "the lane without rotations vs a lane of the existing batch entry")
    assert not all(np.array_equal(x, y) for x, y in zip(plain[0], got[0]))      # ... and the rotations of the others are live
    assert not all(np.array_equal(x, y) for x, y in zip(plain[1], got[1]))


def test_batch_flush_ends_every_lanes_stream(B):
    """rebvio_hip_batch_flush in mid-stream, with rotations: unlike a context's flush it ends every lane's stream (lock-step). Each
    lane equals a stand-alone context run over the frames before the flush and a FRESH one over the frames behind it, whose first
    rotation is ignored; the pair across the flush does not exist."""
    from rebvio_amd import synth
    W, H, L, cut = 192, 144, 2, 8
    order = synth.pingpong_indices(12, 16)
    cam = synth.render_stream(W, H, 1)[1]
    seqs = [np.ascontiguousarray(synth.render_stream(W, H, 12, stream_id=l)[0][order]) for l in range(L)]
    rots = [gyro_rotations(order, 5, 0), [None] * len(order)]
    b = B.Batch(params_for(B, cam), L)
    devs = [b.lanes[l].upload_frames(seqs[l]) for l in range(L)]
    recs = [[] for _ in range(L)]

    def take(outs, ns):
        for l in range(L):
            if outs[l].status >= 0:
                recs[l].append(rec(outs[l], ns[l]))

    for k in range(len(order)):
        take(*b.push_px_gyro_device([devs[l] + k * W * H for l in range(L)], B.PX_GRAY8, [rots[l][k] for l in range(L)], None, k * TS))
        if k + 1 == cut:
            for outs, ns in b.flush():
                take(outs, ns)
    for outs, ns in b.flush():
        take(outs, ns)
    b.close()
    for l in range(L):
        assert len(recs[l]) == len(order) - 2
        # (a stand-alone context carries its detector's servo state from one segment into the next, like a lane does: one context,
        # its gyro stream ended between the segments by rebvio_hip_reset_state + the state put back)
        ctx = B.Context(params_for(B, cam))
        dev = ctx.upload_frames(seqs[l])
        want = []
        for k in range(len(order)):
            out, n = ctx.push_frame_px_gyro_device(dev + k * W * H, B.PX_GRAY8, rots[l][k], None, k * TS)
            if out.status >= 0:
                want.append(rec(out, n))
            if k + 1 == cut:
                want.extend(rec(o, n) for o, n in ctx.flush())
                bg, wbg = ctx.gyro_state()
                ctx.reset_state()
                ctx.set_gyro_state(bg, wbg)
        want.extend(rec(o, n) for o, n in ctx.flush())
        ctx.close()
        same_records(want, recs[l], f"lane {l}")


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------
def test_non_finite_rotations_are_refused_and_leave_no_trace(request, orc_mod, B):
    c = case(request, orc_mod, B, "small")
    cam, seq, R = c["cam"], c["seq"], c["R"]
    npx = cam.width * cam.height
    ctx = B.Context(params_for(B, cam))
    dev = ctx.upload_frames(seq)
    for bad in (np.nan, np.inf, -np.inf):
        Rb = R[1].copy()
        Rb[1, 2] = bad
        with pytest.raises(B.HipError, match=r"error -3.*R_gyro"):
            ctx.push_frame_px_gyro_device(dev, B.PX_GRAY8, Rb, None, 0)
        with pytest.raises(B.HipError, match=r"error -3.*R_gyro"):
            ctx.push_frame_px_gyro(np.ascontiguousarray(seq[0]), B.PX_GRAY8, Rb, 0)
    assert ctx.pairs_started() == 0
    got = []
    for k in range(len(seq)):
        if k == 8:                                       # ... and in the middle of a stream
            Rb = R[8].copy()
            Rb[0, 0] = np.nan
            with pytest.raises(B.HipError, match=r"error -3.*R_gyro"):
                ctx.push_frame_px_gyro_device(dev + k * npx, B.PX_GRAY8, Rb, None, k * TS)
        out, n = ctx.push_frame_px_gyro_device(dev + k * npx, B.PX_GRAY8, R[k], None, k * TS)
        if out.status >= 0:
            got.append(rec(out, n))
    got.extend(rec(o, n) for o, n in ctx.flush())
    st = state_words(ctx.gyro_state())
    ctx.close()
    same_records(c["pairs"], got, "stream around refused calls")
    assert np.array_equal(st, c["state"])
    # the batch entry: refused before any lane is touched, the batch stays usable and in lock-step
    b = B.Batch(params_for(B, cam), 2)
    devs = [b.lanes[l].upload_frames(seq) for l in range(2)]
    for bad in (np.nan, np.inf):
        Rb = R[1].copy()
        Rb[2, 2] = bad
        with pytest.raises(B.HipError, match=r"error -3.*R_gyro"):
            b.push_px_gyro_device([devs[0], devs[1]], B.PX_GRAY8, [R[0], Rb], None, 0)
    recs = []
    for k in range(len(seq)):
        outs, ns = b.push_px_gyro_device([devs[l] + k * npx for l in range(2)], B.PX_GRAY8, [R[k], R[k]], None, k * TS)
        if outs[1].status >= 0:
            recs.append(rec(outs[1], ns[1]))
    for outs, ns in b.flush():
        recs.append(rec(outs[1], ns[1]))
    b.close()
    same_records(c["pairs"], recs, "batch lane around a refused call")
