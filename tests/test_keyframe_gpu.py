"""Keyframes: rebvio_hip_map_mark_keyframe, rebvio_hip_keyframe_next and rebvio_hip_map_keyframe_matches.

Every keyline carries match_id_keyframe (types/keyline.hpp:39); forwardMatch and directedMatch copy it from the matched keyline of
the old map (edge_map.cpp:93,210) and directedMatch counts the survivors into kf_matches (edge_map.cpp:212). Marking a map
(match_id_keyframe[i] = i) starts that propagation; the correspondences entry reads it out. The contracts:
  - a mark changes match_id_keyframe and nothing else;
  - after a mark the library and the CPU oracle (whose map is given the same ids with set_keylines) agree on every pair in every
    word of the record and every field of every keyline, kf_matches and match_id_keyframe included;
  - a stream with rebvio_hip_keyframe_next in front of frame j equals the per-pair run track_pair(j-1, j); mark(j); track_pair(j, j+1)
    in every word, whatever the pipeline's shape;
  - the correspondences equal np_kf_matches, a numpy restatement, applied to the keylines downloaded just before.
All streams are 160x120 with keylines_max 800 (every map is truncated to exactly 800 keylines) unless a case says otherwise."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import params_for
from support import B, refusal_scene  # noqa: F401
from support import DEAD_MAP, assert_refused
from support import (F32, KF_MATCH_DTYPE, TS, assert_keylines_equal, gyro_rotations, np_kf_matches, rec, same_records, set_forms,
                     state_words, vision_only_fusion)

pytestmark = pytest.mark.gpu

W, H, NF = 160, 120, 10
KW = dict(keylines_ref=600, keylines_max=800, global_min_matches_threshold=50)


@pytest.fixture(scope="module", autouse=True)
def binding_record_is_the_restatements(B):
    assert B.KF_MATCH_DTYPE == KF_MATCH_DTYPE


@functools.lru_cache(maxsize=None)
def stream():
    """ten frames of the 160x120 synthetic stream, their camera, and one gyro rotation per frame (as test_stream_gyro_gpu.py)"""
    from rebvio_amd import synth
    frames, cam = synth.render_stream(W, H, NF)
    return frames, cam, gyro_rotations(np.arange(NF), 5)


def assert_matches_equal(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in KF_MATCH_DTYPE.names:
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        assert a.tobytes() == b.tobytes(), (what, f, np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(len(a), -1).any(1))[:8])


def sized_map(B, n, frame=1):
    """(context, map) with exactly n keylines: keylines_max = n truncates the frame's keylines (n = 0: a blank frame)"""
    frames, cam, _ = stream()
    if n == 0:
        ctx = B.Context(params_for(B, cam, **KW))
        m = ctx.detect_u8(np.full((H, W), 128, np.uint8), 0)
    else:
        ctx = B.Context(params_for(B, cam, keylines_ref=max(1, n - 1), keylines_max=n, global_min_matches_threshold=1))
        m = ctx.detect_u8(frames[frame], 0)
    assert m.size() == n, (n, m.size())
    return ctx, m


# ---- 1. the mark ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 257])
def test_mark_sets_the_ids_and_nothing_else(B, n):
    """the wave and workgroup edges of k_mark_keyframe; a second mark changes nothing"""
    ctx, m = sized_map(B, n)
    before = m.keylines()
    if n:
        assert (before["match_id_keyframe"] == -1).all()
    for _ in range(2):
        m.mark_keyframe()
        after = m.keylines()
        assert np.array_equal(after["match_id_keyframe"], np.arange(n))
        assert_keylines_equal(before, after, f"n = {n}", skip=("match_id_keyframe",))
    ctx.close()


def test_mark_with_keylines_max_above_the_map_size(B):
    """n < keylines_max through a detection mask: the slots behind the map's size stay untouched (an upload of more keylines is not
    possible, so the check is on the keylines themselves, and on a second map of the pool that was never marked)"""
    frames, cam, _ = stream()
    ctx = B.Context(params_for(B, cam, **KW))
    mask = np.zeros((H, W), np.uint8)
    mask[20:70, 30:110] = 1
    ctx.set_detection_mask(mask)
    m, other = ctx.detect_u8(frames[1], 0), ctx.detect_u8(frames[2], TS)
    n = m.size()
    assert 64 < n < KW["keylines_max"], n           # (405 keylines of this frame lie inside the mask)
    before, other_before = m.keylines(), other.keylines()
    m.mark_keyframe()
    after = m.keylines()
    assert np.array_equal(after["match_id_keyframe"], np.arange(n))
    assert_keylines_equal(before, after, "masked map", skip=("match_id_keyframe",))
    assert_keylines_equal(other_before, other.keylines(), "the unmarked map")
    ctx.close()


# ---- 2. propagation against the oracle -------------------------------------------------------------------------------------------
def _oracle_mark(m):
    kl = m.keylines()
    kl["match_id_keyframe"] = np.arange(len(kl))
    m.set_keylines(kl)


def _propagation(orc_mod, B, marks, pairs=6):
    """`pairs` pairs through the per-pair API on both sides; marks: the frames whose map is marked (after it was a pair's new map,
    before it is an old map). Returns the oracle's kf_matches per pair."""
    frames, cam, _ = stream()
    orc = orc_mod.Oracle(params_for(orc_mod, cam, **KW))
    orc.set_sum_order("device")
    gpu = B.Context(params_for(B, cam, **KW))
    mo, mg, kf = [], [], []
    for k in range(pairs + 1):
        mo.append(orc.detect_u8(frames[k], k * TS))
        mg.append(gpu.detect_u8(frames[k], k * TS))
        if len(mo) > 2:
            mo.pop(0)
            mg.pop(0).release()
        if k:
            po, pg = orc.track_pair(mo[0], mo[1]), gpu.track_pair(mg[0], mg[1])
            print("pair", k - 1, "keylines", mo[1].size(), "klm_num", po.klm_num, "kf_matches", po.kf_matches, "/", pg.kf_matches)
            assert po.status == 0
            assert np.array_equal(rec(po, mo[1].size()), rec(pg, mg[1].size())), (k, po.kf_matches, pg.kf_matches)
            assert_keylines_equal(mo[1].keylines(), mg[1].keylines(), f"new map of pair {k - 1}")
            kf.append(po.kf_matches)
        if k in marks:
            _oracle_mark(mo[-1])
            mg[-1].mark_keyframe()
            assert_keylines_equal(mo[-1].keylines(), mg[-1].keylines(), f"map {k} after its mark")
    gpu.close()
    return kf


def test_ids_propagate_as_in_the_oracle(orc_mod, B):
    kf = _propagation(orc_mod, B, marks=(0,))
    assert all(v >= 1 for v in kf[:3]), kf          # the precondition, on the oracle alone (measured: 774, 744, 719)
    assert kf[0] > 500 and kf == sorted(kf, reverse=True), kf


def test_a_second_mark_restarts_the_ids(orc_mod, B):
    """marked again at frame 3: the pair behind it counts the survivors of THAT map (more than the first keyframe would still have)"""
    once = _propagation(orc_mod, B, marks=(0,))
    twice = _propagation(orc_mod, B, marks=(0, 3))
    assert once[:3] == twice[:3] and twice[3] > once[3] and twice[3] > twice[2], (once, twice)


# ---- 3. the streaming driver -------------------------------------------------------------------------------------------------------
_ref = {}


def pairs_ref(B, mark_at, gyro):
    """per-pair reference, computed once: track_pair(k-1, k, R[k]) and the mark of frame mark_at (None: no mark) behind the pair that
    ends at it. (records as words, gyro state, size of the marked map)"""
    if (mark_at, gyro) not in _ref:
        frames, cam, R = stream()
        ctx = B.Context(params_for(B, cam, **KW))
        dev = ctx.upload_frames(frames)
        maps, recs = [], []
        for k in range(NF):
            maps.append(ctx.detect_u8_device(dev + k * W * H, k * TS))
            if len(maps) > 2:
                maps.pop(0).release()
            if k:
                recs.append(rec(ctx.track_pair(maps[0], maps[1], R_prior=R[k] if gyro else None), maps[1].size()))
            if k == mark_at:
                maps[-1].mark_keyframe()
        st = state_words(ctx.gyro_state())
        ctx.close()
        _ref[(mark_at, gyro)] = (recs, st)
    return _ref[(mark_at, gyro)]


def kf_words(recs):
    """kf_matches of every record (support.rec: the record's words, then the keyline count; kf_matches is the fifth word from the end of
    the record: kf_matches, reg_num, lm_accept_mask, status)"""
    return [int(r[-5].view(np.int32)) for r in recs]


def run_stream(B, requests=(), gyro=False, flush_after=(), reset_after_request=False, profile=False, order=None):
    """the streaming driver over the ten frames (or frames[order]); requests: frame counts in front of which keyframe_next is called"""
    frames, cam, R = stream()
    order = np.arange(NF) if order is None else order
    ctx = B.Context(params_for(B, cam, **KW))
    dev = ctx.upload_frames(frames)
    if profile:
        ctx.profile_reset()
        ctx.profile(True)
    recs = []
    for k, i in enumerate(order):
        if k in requests:
            ctx.keyframe_next()
            if reset_after_request:
                ctx.reset_state()
        if gyro:
            out, n = ctx.push_frame_px_gyro_device(dev + int(i) * W * H, B.PX_GRAY8, R[k], None, k * TS)
        else:
            out, n = ctx.push_frame_u8_device(dev + int(i) * W * H, k * TS)
        if out.status >= 0:
            recs.append(rec(out, n))
        if k + 1 in flush_after:
            recs.extend(rec(o, n) for o, n in ctx.flush())
    recs.extend(rec(o, n) for o, n in ctx.flush())
    st = state_words(ctx.gyro_state())
    launches = None
    if profile:
        launches = {name: calls for name, (_, calls) in ctx.profile_read().items()}
        ctx.profile(False)
    ctx.close()
    return recs, st, launches


def test_the_reference_runs_carry_keyframe_matches(B):
    """what the streaming cases compare against is worth comparing: no mark, no kf_matches; a mark, and every pair behind it has some"""
    assert kf_words(pairs_ref(B, None, False)[0]) == [0] * (NF - 1)
    for gyro in (False, True):
        assert all(v > 300 for v in kf_words(pairs_ref(B, 0, gyro)[0]))
        kf = kf_words(pairs_ref(B, 3, gyro)[0])
        assert kf[:3] == [0, 0, 0] and all(v > 300 for v in kf[3:]), kf


@pytest.mark.parametrize("gyro", [False, True], ids=["plain", "gyro"])
@pytest.mark.parametrize("mark_at", [0, 3])
@pytest.mark.parametrize("env", [dict(REBVIO_HIP_LEAD="3", REBVIO_HIP_GROUP="1"), dict(REBVIO_HIP_LEAD="5", REBVIO_HIP_GROUP="4"),
                                 dict(REBVIO_HIP_LEAD="8", REBVIO_HIP_GROUP="2"), dict(REBVIO_HIP_LEAD="12", REBVIO_HIP_GROUP="6"),
                                 dict(REBVIO_HIP_LM="seq"), dict(REBVIO_HIP_LM="spec")],
                         ids=["lead3-group1", "lead5-group4", "lead8-group2", "lead12-group6", "lm-seq", "lm-spec"])
def test_keyframe_next_equals_the_per_pair_mark(B, monkeypatch, env, mark_at, gyro):
    want, st = pairs_ref(B, mark_at, gyro)
    set_forms(monkeypatch, **env)
    got, sg, _ = run_stream(B, requests=(mark_at,), gyro=gyro)
    same_records(want, got, f"{env} mark at {mark_at}")
    assert np.array_equal(st, sg)


@pytest.mark.parametrize("flush_after", [(4,), (6,), (1, 2, 6, 9)], ids=["behind-the-mark", "at-the-mark", "many"])
def test_gyro_stream_carries_the_request_across_a_flush(B, monkeypatch, flush_after):
    """keyframe_next in front of frame 5 of a gyro stream that is flushed around it. Flushed right behind frame 5 (six frames in)
    the flagged map is the one the stream carries across the flush: it keeps the flag and is marked in front of pair (5, 6)."""
    set_forms(monkeypatch, REBVIO_HIP_LEAD="3", REBVIO_HIP_GROUP="1")
    want, st = pairs_ref(B, 5, True)
    got, sg, _ = run_stream(B, requests=(5,), gyro=True, flush_after=flush_after)
    same_records(want, got, f"flush after {flush_after}")
    assert np.array_equal(st, sg)
    kf = kf_words(got)
    assert kf[:5] == [0] * 5 and all(v > 300 for v in kf[5:]), kf


def test_a_flagged_frame_dropped_at_a_flush_leaves_no_flag_in_the_pool(B, monkeypatch):
    """A stream without rotations ends at its flush and its newest map goes back to the pool untracked as an old map - with the
    request it carried. With lead 3 / group 1 the pool holds nine maps: the fourteen frames of the second stream reuse every one of
    them, the once-flagged map as an old map too; none of its pairs may see a keyframe id."""
    from rebvio_amd import synth
    set_forms(monkeypatch, REBVIO_HIP_LEAD="3", REBVIO_HIP_GROUP="1")
    order = synth.pingpong_indices(NF, 20)
    want, st, _ = run_stream(B, flush_after=(6,), order=order)
    got, sg, _ = run_stream(B, requests=(5,), flush_after=(6,), order=order)
    assert len(want) == 5 + 13
    same_records(want, got, "request on the last frame in front of a flush")
    assert np.array_equal(st, sg)
    assert kf_words(got) == [0] * 18


def test_streams_without_a_request_launch_what_they_launched_before(B):
    """no request: the per-pair records without a mark, and no k_mark_keyframe launch; one request: the same launches plus exactly one
    k_mark_keyframe; a request dropped by reset_state: the same launches again."""
    want, st = pairs_ref(B, None, False)
    plain, sp, launches = run_stream(B, profile=True)
    same_records(want, plain, "no request vs track_pair")
    assert np.array_equal(st, sp)
    assert "k_mark_keyframe" not in launches and sum(launches.values()) > 4 * NF, launches
    marked, _, lm = run_stream(B, requests=(3,), profile=True)
    assert lm == dict(launches, k_mark_keyframe=1), (lm, launches)
    assert not all(np.array_equal(x, y) for x, y in zip(plain, marked))
    dropped, sd, ld = run_stream(B, requests=(0,), reset_after_request=True, profile=True)
    same_records(plain, dropped, "request dropped by reset_state")
    assert np.array_equal(sp, sd) and ld == launches, (ld, launches)


def test_a_batch_lane_refuses_the_request(B):
    _, cam, _ = stream()
    bat = B.Batch(params_for(B, cam, **KW), 2)
    for lane in bat.lanes:
        with pytest.raises(B.HipError, match=r"error -3.*lane of a batch"):
            lane.keyframe_next()
    bat.close()
    assert B.lib().rebvio_hip_keyframe_next(None) == -3


# ---- 4. correspondences ------------------------------------------------------------------------------------------------------------
def test_matches_of_a_map_four_pairs_after_its_keyframe(B):
    frames, cam, _ = stream()
    ctx = B.Context(params_for(B, cam, **KW))
    maps = [ctx.detect_u8(frames[k], k * TS) for k in range(5)]
    n0 = maps[0].size()
    maps[0].mark_keyframe()
    for k in range(4):
        assert ctx.track_pair(maps[k], maps[k + 1]).status == 0
    kl = maps[4].keylines()
    want, count = np_kf_matches(kl, n0)
    got, n = maps[4].keyframe_matches(n0, return_count=True)
    print("keyframe", n0, "keylines; four pairs on:", count, "of them alive,", int(want["claimants"].sum()), "claimants, most on one:", int(want["claimants"].max()))
    assert n == count and 100 < count < n0 and want["claimants"].max() > 1
    assert_matches_equal(got, want, "four pairs on")
    assert np.all(np.diff(got["kf_keyline"]) > 0)
    again = maps[4].keyframe_matches(n0)
    assert again.tobytes() == got.tobytes()                     # two calls in a row
    assert_keylines_equal(kl, maps[4].keylines(), "the map itself")  # ... and the map is only read
    ctx.close()


SIGMAS = np.array([0.5, 0.5, 0.25, 0.25, np.nan, -1.0, -0.0, 0.0, np.inf, -np.inf, 1e-3, 3.0], F32)


def crafted(kl, kf_size, kmax, mode, seed):
    """keyline array with crafted keyframe ids and sigma_rho. "slot0": every keyline claims slot 0; "ties": few slots, sigma_rho from
    a handful of values (equal ones among the claimants of a slot: the index decides; NaN, negative, -0.0, +-inf); "edges": the ids
    -1, kf_size - 1, kf_size, keylines_max and INT_MIN / INT_MAX next to random ones"""
    rng = np.random.default_rng(seed)
    kl = kl.copy()
    n = len(kl)
    kl["sigma_rho"] = SIGMAS[rng.integers(0, len(SIGMAS), n)]
    kl["rho"] = rng.uniform(0.01, 5.0, n).astype(F32)
    kl["matches"] = rng.integers(0, 20, n).astype(np.uint32)
    if mode == "slot0":
        kl["match_id_keyframe"] = 0
    elif mode == "ties":
        kl["match_id_keyframe"] = rng.integers(0, max(1, min(kf_size, 5)), n)
    else:
        special = np.array([-1, kf_size - 1, kf_size, kmax, -2 ** 31, 2 ** 31 - 1, 0], np.int64)
        ids = np.where(rng.random(n) < 0.5, special[rng.integers(0, len(special), n)], rng.integers(-1, kmax + 2, n))
        kl["match_id_keyframe"] = ids.astype(np.int32)
    return kl


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_matches_of_crafted_maps(B, n):
    ctx, m = sized_map(B, n)       # (keylines_max = n)
    base = m.keylines()
    for mode in ("slot0", "ties", "edges"):
        for kf_size in sorted({0, 1, n}):
            kl = crafted(base, kf_size, n, mode, 17 * n + kf_size)
            m.upload(kl)
            assert_keylines_equal(kl, m.keylines(), "upload")
            want, count = np_kf_matches(kl, kf_size)
            got, cnt = m.keyframe_matches(kf_size, return_count=True)
            assert cnt == count, (mode, kf_size, cnt, count)
            assert_matches_equal(got, want, f"n {n} {mode} kf_size {kf_size}")
            if mode == "slot0" and kf_size:
                assert count == 1 and got[0]["claimants"] == n
    ctx.close()


def test_matches_with_keylines_max_above_the_map_size(B):
    """n < keylines_max (a detection mask keeps the map small): kf_size up to keylines_max, ids of kf_size and keylines_max"""
    frames, cam, _ = stream()
    ctx = B.Context(params_for(B, cam, **KW))
    mask = np.zeros((H, W), np.uint8)
    mask[20:70, 30:110] = 1
    ctx.set_detection_mask(mask)
    m = ctx.detect_u8(frames[1], 0)
    n, kmax = m.size(), KW["keylines_max"]
    assert 256 < n < kmax, n
    base = m.keylines()
    seen = 0
    for mode in ("slot0", "ties", "edges"):
        for kf_size in (0, 1, n, kmax):
            kl = crafted(base, kf_size, kmax, mode, 5 + kf_size)
            m.upload(kl)
            want, count = np_kf_matches(kl, kf_size)
            got, cnt = m.keyframe_matches(kf_size, return_count=True)
            assert cnt == count, (mode, kf_size, cnt, count)
            assert_matches_equal(got, want, f"{mode} kf_size {kf_size}")
            seen = max(seen, count)
    assert seen > 64
    ctx.close()


def test_cap_below_count_and_a_null_buffer(B):
    ctx, m = sized_map(B, 257)
    kl = crafted(m.keylines(), 257, 257, "edges", 3)
    m.upload(kl)
    want, count = np_kf_matches(kl, 257)
    assert count > 40
    L = B.lib()
    cap, guard = count // 3, 16
    buf = np.full((cap + guard) * 32, 0xA5, np.uint8)
    n = C.c_int(-1)
    assert L.rebvio_hip_map_keyframe_matches(m.h, 257, buf.ctypes.data_as(C.POINTER(B.KfMatch)), cap, C.byref(n)) == 0
    assert n.value == count
    assert buf[:cap * 32].tobytes() == want[:cap].tobytes()
    assert (buf[cap * 32:] == 0xA5).all(), "records written beyond cap"
    n = C.c_int(-1)
    assert L.rebvio_hip_map_keyframe_matches(m.h, 257, None, 0, C.byref(n)) == 0 and n.value == count
    got, cnt = m.keyframe_matches(257, cap=10 ** 6, return_count=True)    # a cap above keylines_max
    assert cnt == count
    assert_matches_equal(got, want, "large cap")
    ctx.close()


def test_an_empty_map_has_no_matches(B):
    ctx, m = sized_map(B, 0)
    for kf_size in (0, 1, KW["keylines_max"]):
        got, cnt = m.keyframe_matches(kf_size, return_count=True)
        assert cnt == 0 and len(got) == 0
    ctx.close()


# ---- 5. refusals and leaks ---------------------------------------------------------------------------------------------------------
def test_refusals(B):
    frames, cam, _ = stream()
    ctx, other = B.Context(params_for(B, cam, **KW)), B.Context(params_for(B, cam, **KW))
    maps = [ctx.detect_u8(frames[k], k * TS) for k in range(3)]
    foreign = other.detect_u8(frames[0], 0)
    L = B.lib()
    n = C.c_int()
    rec = (B.KfMatch * 4)()
    err = lambda: L.rebvio_hip_last_error().decode()
    assert L.rebvio_hip_map_mark_keyframe(None, maps[0].h) == -3 and "null" in err()
    assert L.rebvio_hip_map_mark_keyframe(ctx.h, None) == -3 and "null" in err()
    assert L.rebvio_hip_map_mark_keyframe(ctx.h, foreign.h) == -3 and "another context" in err()
    assert L.rebvio_hip_map_keyframe_matches(None, 1, rec, 4, C.byref(n)) == -3 and "null map" in err()
    assert L.rebvio_hip_map_keyframe_matches(maps[0].h, 1, rec, 4, None) == -3 and "null count" in err()
    assert L.rebvio_hip_map_keyframe_matches(maps[0].h, 1, rec, -1, C.byref(n)) == -3 and "cap" in err()
    assert L.rebvio_hip_map_keyframe_matches(maps[0].h, 1, None, 4, C.byref(n)) == -3 and "output buffer" in err()
    assert L.rebvio_hip_map_keyframe_matches(maps[0].h, -1, rec, 4, C.byref(n)) == -3 and "kf_size" in err()
    assert L.rebvio_hip_map_keyframe_matches(maps[0].h, KW["keylines_max"] + 1, rec, 4, C.byref(n)) == -3 and "kf_size" in err()
    # a map promised to R_prior_next: marked like any other, its correspondences refused until the next _begin has run
    maps[0].mark_keyframe()
    c, s = F32(np.cos(0.01)), F32(np.sin(0.01))
    Rn = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], F32)
    mid = ctx.track_pair_begin(maps[0], maps[1])
    ctx.track_pair_finish_async(maps[0], maps[1], *vision_only_fusion(mid), R_prior_next=Rn)
    assert ctx.track_pair_result()[3] == 0
    with pytest.raises(B.HipError) as e:
        maps[1].keyframe_matches(maps[0].size())
    assert "error -7:" in str(e.value) and "R_prior_next" in str(e.value), str(e.value)
    maps[1].mark_keyframe()
    mid = ctx.track_pair_begin(maps[1], maps[2], R_prior=Rn)
    ctx.track_pair_finish_async(maps[1], maps[2], *vision_only_fusion(mid))
    klm, kf, _, status = ctx.track_pair_result()
    assert status == 0 and kf > 0, (klm, kf, status)
    kl = maps[2].keylines()
    want, count = np_kf_matches(kl, maps[1].size())
    assert_matches_equal(maps[1 + 1].keyframe_matches(maps[1].size()), want, "after the next begin")
    assert maps[1].keyframe_matches(maps[1].size(), cap=0, return_count=True)[1] == maps[1].size()   # the keyframe against itself
    gone = C.c_void_p(ctx.h.value)       # (compared with the map's context, never dereferenced: the map's life block says it is gone)
    ctx.close()
    other.close()
    assert L.rebvio_hip_map_mark_keyframe(gone, maps[0].h) == -10 and "destroyed" in err()
    assert L.rebvio_hip_map_keyframe_matches(maps[0].h, 1, rec, 4, C.byref(n)) == -10 and "destroyed" in err()
    for m in maps + [foreign]:
        m.release()


def test_every_new_entry_gives_its_resources_back(B):
    frames, cam, _ = stream()
    live = B.test_live_resources()
    ctx = B.Context(params_for(B, cam, **KW))
    dev = ctx.upload_frames(frames)
    maps = [ctx.detect_u8_device(dev + k * W * H, k * TS) for k in range(2)]
    maps[0].mark_keyframe()
    assert ctx.track_pair(maps[0], maps[1]).kf_matches > 300
    base = B.test_live_resources()
    assert len(maps[1].keyframe_matches(maps[0].size())) > 300
    assert B.test_live_resources() == base + 2                  # slot table and record buffer, allocated on first use ...
    maps[1].keyframe_matches(maps[0].size())
    assert B.test_live_resources() == base + 2                  # ... and kept
    for m in maps:
        m.release()
    ctx.keyframe_next()
    for k in range(2, NF):
        ctx.push_frame_u8_device(dev + k * W * H, k * TS)
    assert len(ctx.flush()) >= 1
    ctx.keyframe_next()
    ctx.close()
    assert B.test_live_resources() == live


# ---- the refusal table: every shared refusal with its code and whole text; which one wins when several apply ------
_mark = lambda s, m: s.B.lib().rebvio_hip_map_mark_keyframe(s.other.h, m.h)
_snapshot = lambda s, m: s.B.lib().rebvio_hip_map_keyframe_snapshot(s.other.h, m.h, C.byref(C.c_void_p()))
REFUSED = {
    "mark: map of another context": (lambda s: _mark(s, s.m), -3, "map_mark_keyframe: map of another context"),
    "mark: wins: a destroyed map over another context": (lambda s: _mark(s, s.dm), -10, DEAD_MAP),
    "snapshot: map of another context": (lambda s: _snapshot(s, s.m), -3, "map_keyframe_snapshot: map of another context"),
    "snapshot: wins: a destroyed map over another context": (lambda s: _snapshot(s, s.dm), -10, DEAD_MAP),
}
@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusal_table(refusal_scene, case):
    """every refusal of the table with its return code and its whole rebvio_hip_last_error text; nothing is allocated"""
    assert_refused(refusal_scene, *REFUSED[case])
