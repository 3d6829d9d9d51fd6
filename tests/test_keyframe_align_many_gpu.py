"""Many hypotheses against one map on the device: rebvio_hip_map_keyframe_align_many (k_kf_align_sums_many, k_kf_pose_step_many).
The yardstick is rebvio_hip_map_keyframe_align, whose kernels this change leaves as they are: for every hypothesis the pose block is
the single entry's for the same snapshot, guess and options, byte for byte - with uneven sizes in one call (a hypothesis's idle
workgroups), with 1, 2 and 64 hypotheses, with and without normals, next to empty snapshots, next to status 2 and 3, and through the
256-partial sum with blockIdx.y > 0. inliers is the numpy count of used terms with |e| <= huber_px at the returned pose, compared
only where no term of the restatement comes within GUARD of the Huber switch, a cell edge or the gate. The launch count does not
depend on n; the scratch is one allocation; every refusal comes before the device is touched; tracking is not disturbed.
Snapshots are crafted (tests/kf_align_many_ref.py: Scene800) on the 160x120 stream with keylines_max 800 unless a case says otherwise."""
import ctypes as C

import numpy as np
import pytest

from conftest import params_for
from kf_align_many_ref import Scene800, cam_of, current_data, np_inliers, seeded_guesses, stream
from kf_align_ref import GUARD, OFFSETS, craft_against, craft_kf_keylines, offset_guess
from kf_pose_ref import true_motion
from support import B, refusal_scene  # noqa: F401
from support import DEAD_MAP, DEAD_SNAPSHOT, assert_refused, foreign_snapshot, no_field
from support import F32, TS, assert_keylines_equal, enlarged_stream, rec, same_records, vision_only_fusion

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 800)
KW_STREAM = dict(keylines_ref=600, keylines_max=800, global_min_matches_threshold=50)      # the stream of the pose tests: every pair tracks


@pytest.fixture(scope="module")
def scene(B):
    """the scene and one snapshot per size of SIZES (with normals), shared by the tests below and left unchanged by them"""
    S = Scene800(B)
    S.by_size = {n: S.snapshot(n) for n in SIZES}
    yield S
    S.close()


def hyps_of(B, items):
    """[(snapshot, R0, t0)] -> KfHypothesis list"""
    return [B.kf_hypothesis(s, R0, t0) for s, R0, t0 in items]


def assert_same_as_single(B, mc, items, res, opts, what):
    assert len(res) == len(items)
    for k, ((s, R0, t0), r) in enumerate(zip(items, res)):
        one = mc.keyframe_align(s, opts, R0, t0)
        assert bytes(r.pose) == bytes(one), (what, k, r.pose.status, one.status, r.pose.used, one.used)
        assert 0 <= r.inliers <= r.pose.used and r.reserved == 0, (what, k)


# ---- 1. bit parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", [0, 8])
def test_uneven_sizes_in_one_call(B, scene, max_iter):
    """snapshots of 1 .. 800 keylines together: the grid is (4, 8) and all but the largest hypothesis have workgroups that leave at
    once; then reversed, the largest first"""
    guesses = seeded_guesses(len(SIZES), 21, *true_motion())
    items = [(scene.by_size[n][0], *g) for n, g in zip(SIZES, guesses)]
    opts = B.default_kf_align_opts(scene.ctx, max_iter=max_iter)
    res = scene.mc.keyframe_align_many(hyps_of(B, items), opts)
    assert [r.pose.candidates for r in res] == list(SIZES)
    assert_same_as_single(B, scene.mc, items, res, opts, f"max_iter {max_iter}")
    assert res[-1].pose.status == 0 and res[-1].pose.used >= 12 and res[0].pose.status == 3
    back = scene.mc.keyframe_align_many(hyps_of(B, items[::-1]), opts)
    assert [bytes(r) for r in back] == [bytes(r) for r in res[::-1]]


def test_one_two_and_64_hypotheses_on_one_snapshot(B, scene):
    snap = scene.by_size[800][0]
    guesses = seeded_guesses(64, 22, *true_motion())
    items = [(snap, *g) for g in guesses]
    opts = B.default_kf_align_opts(scene.ctx)
    res = {n: scene.mc.keyframe_align_many(hyps_of(B, items[:n]), opts) for n in (1, 2, 64)}
    assert_same_as_single(B, scene.mc, items, res[64], opts, "64")
    for n in (1, 2):
        assert [bytes(r) for r in res[n]] == [bytes(r) for r in res[64][:n]], n
    again = scene.mc.keyframe_align_many(hyps_of(B, items), opts)
    assert [bytes(r) for r in again] == [bytes(r) for r in res[64]]
    assert all(r.pose.status == 0 and r.pose.iterations == 8 for r in res[64])
    assert len({bytes(r.pose) for r in res[64]}) == 64           # 64 different answers: no hypothesis read another's state


@pytest.mark.parametrize("min_used", [12, 0])
def test_mixed_list_with_and_without_normals_and_an_empty_snapshot(B, scene, min_used):
    with_n = scene.by_size[257][0]
    bare, _ = scene.snapshot(257, normals=False)
    empty, _ = scene.snapshot(0)
    R0, t0 = offset_guess(*OFFSETS[1])
    R1, t1 = offset_guess(*OFFSETS[0])
    items = [(empty, R1, t1), (with_n, R0, t0), (bare, R0, t0), (empty, R0, t0), (with_n, R1, t1)]
    opts = B.default_kf_align_opts(scene.ctx, min_used=min_used)
    res = scene.mc.keyframe_align_many(hyps_of(B, items), opts)
    assert_same_as_single(B, scene.mc, items, res, opts, f"min_used {min_used}")
    for k, (R, t) in ((0, (R1, t1)), (3, (R0, t0))):
        p = res[k].pose
        assert (p.status, p.candidates, p.used, p.iterations, res[k].inliers) == (3, 0, 0, 0, 0)
        assert np.array_equal(np.array(p.R), R.reshape(9)) and np.array_equal(np.array(p.t), t)
        assert not np.array(p.H).any() and not np.array(p.g).any() and p.cost == 0.0
    assert bytes(res[1].pose) != bytes(res[2].pose)              # the gradient test makes a difference 0.02 rad off
    # an all-empty list launches nothing and still answers
    scene.ctx.profile_reset()
    scene.ctx.profile(True)
    only = scene.mc.keyframe_align_many(hyps_of(B, [items[0], items[3]]), opts)
    launches = {name: calls for name, (_, calls) in scene.ctx.profile_read().items() if calls}
    scene.ctx.profile(False)
    assert launches == {} and [bytes(r) for r in only] == [bytes(res[0]), bytes(res[3])]


def test_statuses_2_and_3_next_to_status_0(B, scene):
    """the good members' bits do not depend on their neighbours: alone, next to a status-3 member (11 keylines, or none that passes
    the filter) and next to a status-2 member (min_used 0 and no term at all: H = 0 does not factor)"""
    good, mid = scene.by_size[800][0], scene.by_size[257][0]
    few, _ = scene.snapshot(11)
    dead, _ = scene.snapshot(64, dead=True)
    R0, t0 = offset_guess(*OFFSETS[0])
    for min_used, want in ((12, [0, 3, 0, 3]), (0, [0, None, 0, 2])):
        opts = B.default_kf_align_opts(scene.ctx, min_used=min_used)
        items = [(good, R0, t0), (few, R0, t0), (mid, R0, t0), (dead, R0, t0)]
        res = scene.mc.keyframe_align_many(hyps_of(B, items), opts)
        assert_same_as_single(B, scene.mc, items, res, opts, f"min_used {min_used}")
        assert all(w is None or r.pose.status == w for r, w in zip(res, want)), [r.pose.status for r in res]
        assert (res[3].pose.used, res[3].inliers, res[3].pose.iterations) == (0, 0, 0)
        alone = scene.mc.keyframe_align_many(hyps_of(B, [items[0], items[2]]), opts)
        assert bytes(alone[0]) == bytes(res[0]) and bytes(alone[1]) == bytes(res[2])


def test_two_hypotheses_over_256_partials(B):
    """keylines_max = 65 536 on a 2304 x 1900 frame, the scene of test_sums_over_256_partials: each of two hypotheses sums 256
    workgroup partials, the second with blockIdx.y = 1"""
    Wb, Hb = 2304, 1900
    frames, cam = enlarged_stream(Wb, Hb, 3)
    ctx = B.Context(B.default_params(Hb, Wb, fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=60000, keylines_max=65536))
    maps = sorted((ctx.detect_u8(frames[i], i * 50000) for i in range(3)), key=lambda x: -x.size())
    mk, mc = maps[0], maps[1]
    assert mk.size() == 65536 and mc.size() > 32768
    kl, cur = current_data(mc)
    A = craft_against(kl, cur[2], cur[3], 5, cam_of(ctx))
    base = mk.keylines()
    base["matches"] = 0
    n = min(len(A["prs4"]), len(base))
    assert n > 32768
    mk.upload(craft_kf_keylines(base, A, n))
    snap = mk.keyframe_snapshot()
    snap.add_normals(mk)
    (Ra, ta), (Rb, tb) = seeded_guesses(2, 3, *true_motion(), rot=0.0005, trans=0.002)
    items = [(snap, Ra, ta), (snap, Rb, tb)]
    for max_iter in (0, 2):
        opts = B.default_kf_align_opts(ctx, max_iter=max_iter)
        res = mc.keyframe_align_many(hyps_of(B, items), opts)
        assert_same_as_single(B, mc, items, res, opts, f"large, max_iter {max_iter}")
        assert all(r.pose.candidates == 65536 and r.pose.used > 1000 for r in res), [r.pose.used for r in res]
        assert bytes(res[0].pose) != bytes(res[1].pose)
    snap.release()
    ctx.close()


# ---- 2. inliers ---------------------------------------------------------------------------------------------------------------------
def test_inliers_against_numpy(B, scene):
    seen = set()
    for opts in (dict(max_iter=0), dict(max_iter=8), dict(max_iter=0, huber_px=0.7, min_cos=0.5, max_dist=6)):
        guesses = [true_motion(), offset_guess(*OFFSETS[0]), offset_guess(*OFFSETS[1]), *seeded_guesses(5, 31, *true_motion())]
        sizes = (800, 257, 800, 65, 800, 256, 63, 255)
        items = [(scene.by_size[n][0], *g) for n, g in zip(sizes, guesses)]
        res = scene.mc.keyframe_align_many(hyps_of(B, items), B.default_kf_align_opts(scene.ctx, **opts))
        kw = {("huber" if k == "huber_px" else k): v for k, v in opts.items() if k != "max_iter"}
        for k, (n, r) in enumerate(zip(sizes, res)):
            inl, used, g = np_inliers(*scene.by_size[n][1], np.array(r.pose.R), np.array(r.pose.t), **kw)
            assert min(g.values()) > GUARD, (opts, k, g)
            assert (r.pose.used, r.inliers) == (used, inl), (opts, k, r.pose.used, used, r.inliers, inl)
            seen.add(inl < used)
    assert seen == {True, False}


# ---- 3. launches and resources -------------------------------------------------------------------------------------------------------
def test_launch_count_does_not_depend_on_n_and_the_scratch_is_one_allocation(B):
    S = Scene800(B)
    snaps = [S.snapshot(n)[0] for n in (65, 257, 800)]
    guesses = seeded_guesses(64, 41, *true_motion())
    base = B.test_live_resources()
    S.ctx.profile_reset()
    S.ctx.profile(True)
    for k, n in enumerate((1, 5, 64)):
        items = [(snaps[i % 3], *guesses[i]) for i in range(n)]
        S.mc.keyframe_align_many(hyps_of(B, items), B.default_kf_align_opts(S.ctx, max_iter=5))
        launches = {name: calls for name, (_, calls) in S.ctx.profile_read().items() if calls}
        assert launches == dict(k_kf_align_sums_many=6, k_kf_pose_step_many=6), (n, launches)
        S.ctx.profile_reset()
        assert B.test_live_resources() == base + 1, n            # the scratch: ONE allocation at the first call, none per call
    S.mc.keyframe_align_many(hyps_of(B, [(snaps[0], *guesses[0])]), B.default_kf_align_opts(S.ctx, max_iter=0))
    launches = {name: calls for name, (_, calls) in S.ctx.profile_read().items() if calls}
    S.ctx.profile(False)
    assert launches == dict(k_kf_align_sums_many=1, k_kf_pose_step_many=1), launches
    S.mc.keyframe_align(snaps[0])                                # the single entry's scratch is its own
    assert B.test_live_resources() == base + 2
    S.close()


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_and_resources(B):
    frames, cam = stream()
    live = B.test_live_resources()
    ctx, other = B.Context(params_for(B, cam, **KW_STREAM)), B.Context(params_for(B, cam, **KW_STREAM))
    maps = [ctx.detect_u8(frames[k], k * TS) for k in range(3)]
    foreign = other.detect_u8(frames[0], 0)
    snap, fsnap = maps[0].keyframe_snapshot(), foreign.keyframe_snapshot()
    snap.add_normals(maps[0])
    L = B.lib()
    err = lambda: L.rebvio_hip_last_error().decode()
    out = (B.KfHypResult * 65)()
    base = B.test_live_resources()

    def arr(items):
        a = (B.KfHypothesis * len(items))()
        for k, h in enumerate(items):
            C.memmove(C.byref(a, k * C.sizeof(B.KfHypothesis)), C.byref(h), C.sizeof(B.KfHypothesis))
        return a
    ok = B.kf_hypothesis(snap)
    many = L.rebvio_hip_map_keyframe_align_many
    assert many(None, arr([ok]), 1, None, out) == -3 and "null" in err()
    assert many(maps[1].h, None, 1, None, out) == -3 and "null" in err()
    assert many(maps[1].h, arr([ok]), 1, None, None) == -3 and "null" in err()
    assert many(maps[1].h, arr([ok]), 0, None, out) == -3 and "n outside" in err()
    assert many(maps[1].h, arr([ok]), -1, None, out) == -3 and "n outside" in err()
    assert many(maps[1].h, arr([ok] * 65), 65, None, out) == -3 and "n outside" in err()
    assert many(maps[1].h, arr([ok, B.kf_hypothesis(None), ok]), 3, None, out) == -3 and "null snapshot" in err()
    assert many(maps[1].h, arr([ok, ok, B.kf_hypothesis(fsnap)]), 3, None, out) == -3 and "another context" in err()
    nan_R = np.eye(3)
    nan_R[2, 0] = np.nan
    for bad in (B.kf_hypothesis(snap, nan_R), B.kf_hypothesis(snap, None, [0.0, 0.0, -np.inf])):
        with pytest.raises(B.HipError, match="error -3:.*non-finite"):
            maps[1].keyframe_align_many([ok, bad])
    sr = int(ctx.p.search_range)
    d = lambda **kw: B.default_kf_align_opts(ctx, **kw)
    for o, word in ((d(huber_px=0.0), "huber_px"), (d(huber_px=float("nan")), "huber_px"), (d(max_iter=33), "max_iter"), (d(max_iter=-1), "max_iter"),
                    (d(min_used=-1), "min_used"), (d(min_used=65537), "min_used"), (d(min_cos=1.5), "min_cos"), (d(min_cos=-1.5), "min_cos"),
                    (d(min_cos=float("nan")), "min_cos"), (d(max_dist=-1), "max_dist"), (d(max_dist=sr + 1), "max_dist"),
                    (d(kf_filter=dict(rho_min=-1.0)), "rho_min"), (d(kf_filter=dict(max_rel_sigma=float("nan"))), "NaN")):
        with pytest.raises(B.HipError) as e:
            maps[1].keyframe_align_many([ok, ok], o)
        assert "error -3:" in str(e.value) and word in str(e.value), str(e.value)
    with pytest.raises(B.HipError, match="error -3:"):
        maps[1].keyframe_align_many([])
    assert B.test_live_resources() == base                      # nothing was allocated by a refused call
    got = maps[1].keyframe_align_many([ok] * 64, d(max_dist=sr, min_cos=1.0, max_iter=32, min_used=65536))
    assert len(got) == 64 and all(r.pose.status == 3 for r in got)         # the bounds themselves are legal
    assert B.test_live_resources() == base + 1
    # a map promised to R_prior_next is accepted, as by the single entry
    c, s = F32(np.cos(0.01)), F32(np.sin(0.01))
    Rn = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], F32)
    mid = ctx.track_pair_begin(maps[0], maps[1])
    ctx.track_pair_finish_async(maps[0], maps[1], *vision_only_fusion(mid), R_prior_next=Rn)
    assert ctx.track_pair_result()[3] == 0
    (r,) = maps[1].keyframe_align_many([ok])
    assert bytes(r.pose) == bytes(maps[1].keyframe_align(snap))
    # an uploaded current map: its field is not detection's - refused as by the single entry
    maps[2].upload(maps[2].keylines())
    with pytest.raises(B.HipError, match="error -7:.*distance field"):
        maps[2].keyframe_align_many([ok])
    ctx.close()
    assert many(maps[1].h, arr([ok]), 1, None, out) == -10 and "destroyed" in err()
    assert many(foreign.h, arr([ok]), 1, None, out) == -10 and "destroyed" in err()
    snap.release()
    fsnap.release()
    other.close()
    for m in maps + [foreign]:
        m.release()
    assert B.test_live_resources() == live


# ---- 5. the real stream ----------------------------------------------------------------------------------------------------------------
def test_align_many_calls_between_pairs_disturb_nothing(B):
    """the pair records and the final keylines of the stream are equal word for word with and without align_many calls between the pairs"""
    frames, cam = stream()

    def run(with_align):
        ctx = B.Context(params_for(B, cam, **KW_STREAM))
        maps = [ctx.detect_u8(frames[k], k * TS) for k in range(9)]
        recs, snaps = [], []
        for k in range(8):
            out = ctx.track_pair(maps[k], maps[k + 1])
            recs.append(rec(out, maps[k + 1].size()))
            if k == 1:
                maps[2].mark_keyframe()          # (marked in both runs: the ids are part of what is compared)
            if k in (1, 3) and with_align:
                snaps.append(maps[k + 1].keyframe_snapshot())
                snaps[-1].add_normals(maps[k + 1])
            if k >= 2 and with_align:
                hyps = [h for s in snaps for h in B.kf_hypotheses_around(s, np.eye(3), np.zeros(3), 0.01, 0.02)]
                res = maps[k + 1].keyframe_align_many(hyps)
                maps[k].keyframe_align_many(hyps[:3])             # an older map too
                best = B.kf_align_best(res, 12)
                print(f"pair {k}: {len(hyps)} hypotheses, best {best}" + (f" inliers {res[best].inliers} of {res[best].pose.used}" if best >= 0 else ""))
        final = maps[8].keylines()
        for s in snaps:
            s.release()
        ctx.close()
        return recs, final

    plain, kl_plain = run(False)
    aligned, kl_aligned = run(True)
    same_records(plain, aligned, "with and without align_many calls")
    assert_keylines_equal(kl_plain, kl_aligned, "final keylines")


# ---- the refusal table: every shared refusal with its code and whole text; which one wins when several apply ------

MANY = "map_keyframe_align_many"
_ao = lambda s, **kw: s.B.default_kf_align_opts(s.ctx, **kw)
_hy = lambda s, *snaps, R0=None: [s.B.kf_hypothesis(sn, R0 if k == len(snaps) - 1 else None, None) for k, sn in enumerate(snaps)]
REFUSED = {
    "destroyed map": (lambda s: s.dm.keyframe_align_many(_hy(s, s.dsnap)), -10, DEAD_MAP),
    "destroyed snapshot, second in the list": (lambda s: s.m.keyframe_align_many(_hy(s, s.snap, s.dsnap)), -10, DEAD_SNAPSHOT),
    "foreign snapshot, second in the list": (lambda s: s.m.keyframe_align_many(_hy(s, s.snap, s.fsnap)), -3, foreign_snapshot(MANY)),
    "no field": (lambda s: s.up.keyframe_align_many(_hy(s, s.snap)), -7, no_field(MANY)),
    "R0 not finite, second in the list": (lambda s: s.m.keyframe_align_many(_hy(s, s.snap, s.snap2, R0=s.nan_R)), -3,
                                          f"{MANY}: non-finite R0 or t0"),
    "min_cos below": (lambda s: s.m.keyframe_align_many(_hy(s, s.snap), _ao(s, min_cos=-1.5)), -3, f"{MANY}: min_cos outside [-1, 1]"),
    "max_dist above": (lambda s: s.m.keyframe_align_many(_hy(s, s.snap), _ao(s, max_dist=s.sr + 1)), -3,
                       f"{MANY}: max_dist outside 0..search_range"),
    "wins: a foreign snapshot over an option and no field": (lambda s: s.up.keyframe_align_many(_hy(s, s.snap, s.fsnap, R0=s.nan_R),
                                                                                               _ao(s, min_cos=2.0)), -3, foreign_snapshot(MANY)),
    "wins: the first of the list, foreign": (lambda s: s.m.keyframe_align_many(_hy(s, s.fsnap, s.dsnap)), -3, foreign_snapshot(MANY)),
    "wins: the first of the list, destroyed": (lambda s: s.m.keyframe_align_many(_hy(s, s.dsnap, s.fsnap)), -10, DEAD_SNAPSHOT),
    "wins: a destroyed map over a foreign snapshot": (lambda s: s.dm.keyframe_align_many(_hy(s, s.snap)), -10, DEAD_MAP),
    "wins: an option over no field": (lambda s: s.up.keyframe_align_many(_hy(s, s.snap), _ao(s, min_cos=2.0)), -3,
                                      f"{MANY}: min_cos outside [-1, 1]"),
}

@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusal_table(refusal_scene, case):
    """every refusal of the table with its return code and its whole rebvio_hip_last_error text; nothing is allocated"""
    assert_refused(refusal_scene, *REFUSED[case])
