"""The entries that go through kfp::lookup (rebvio_amd/csrc/kf_pose.hpp) away from the default context, on the device:
rebvio_hip_map_keyframe_align, _align_many, rebvio_hip_kf_snapshot_fuse_depth and _handover_depth (k_kf_align_sums,
k_kf_align_sums_many, k_kf_fuse_depth, k_kf_handover_claim) on the rows of tests/context_cases.py - a ragged 131x67 frame with a
quarter-pixel principal point, EuRoC's intrinsics over four, a principal point near a corner, search_range 3, 7, 100 and 255 - each on
a map the device detected. Until these cases the kernels' decode of the field key, owner = (mask - (key & mask)) / df_nr and
dist = key >> 23, had run with df_nr = 80 and distances up to 40 only: a literal 80, a cols / 2 for cx or a distance mask one bit too
narrow passed every test. Per row:
  1. the three entries associate the same keylines with the same owners, and that mask is the restatement's on the downloaded field;
     five exits of the lookup and the four sides of the border test are planted (the zero-gradient exit stays with the host half);
  2. one evaluation at the crafted motion and at a seeded guess (assoc exact, the 28 sums within (used + 64) * 2^-52 * sum |term|, a
     second call byte-identical) and one solve against np_kf_align within DEV_VS_NP - the bars of tests/test_keyframe_align_gpu.py;
  3. C and D, the gradient gate off: keylines associated at distances past 40 (C) and from 128 on (D), and a sweep of max_dist;
  4. three hypotheses on two snapshots of unequal size equal the single entry byte for byte, inliers against numpy;
  5. fusion and hand-over against np_kf_fuse / np_kf_handover and the host hook, every word, with claimants that collide;
  6. the defaults and the refusal of max_dist follow the context's search_range;
  7. (A) a lane of a two-lane batch aligns its maps like a stand-alone context.
Everything is exact but the sums and the solve, which keep the bars derived where they were introduced. Non-vacuity is asserted on
the restatement before anything is compared. All maps hold at most 1601 keylines."""
import numpy as np
import pytest

from context_cases import CONTEXTS, IDS, SIDES, DeviceScene, context_params, distance_case, frames_of, successor_records
from kf_align_many_ref import np_inliers, seeded_guesses
from kf_align_ref import (DEV_VS_NP, GUARD, LOOKUP_EXITS, OFFSETS, assert_evaluation, craft_kf_keylines, np_kf_align, np_kf_align_sums,
                          offset_guess, same_bytes)
from kf_fuse_ref import INT_MIN, np_kf_fuse, perturbed
from kf_fuse_ref import counts_of as fuse_counts
from kf_handover_ref import assert_identities, guard_min, np_kf_handover
from kf_handover_ref import counts_of as handover_counts
from kf_pose_ref import pose_err, pose_sums, true_motion
from support import B  # noqa: F401
from support import F32, TS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes(B):
    """one DeviceScene per row, made on first use and shared: its current map is only ever read"""
    made = {}

    def get(cid):
        if cid not in made:
            made[cid] = DeviceScene(B, cid)
        return made[cid]
    yield get
    for s in made.values():
        s.close()


def sr_of(S):
    return int(S.ctx.p.search_range)


# ---- 1. owners ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_alignment_fusion_and_handover_find_the_same_owners(B, scenes, cid):
    S = scenes(cid)
    ctx, mc = S.ctx, S.mc
    src, D, case, want = S.planted()
    assert set(case["plants"]) == set(LOOKUP_EXITS[:5]) and set(case["sides"]) >= {SIDES[1]}
    print(f"{cid}: {len(D[1])} keyframe keylines, {int(want.sum())} associated, max_dist {case['max_dist']}, plants {case['plants']}, "
          f"rim {case['rim']}")
    dst = mc.keyframe_snapshot()
    S.snaps.append(dst)
    R, t = true_motion()
    md = dict(max_dist=case["max_dist"])
    _, align = mc.keyframe_align(src, B.default_kf_align_opts(ctx, max_iter=0, **md), R, t, want_assoc=True)
    _, handover = dst.handover_depth(src, mc, R, t, B.default_kf_handover_opts(ctx, **md), want_assoc=True)       # (src is only read)
    _, fuse = src.fuse_depth(mc, R, t, B.default_kf_fuse_opts(ctx, **md), want_assoc=True)
    a_has, f_has, h_has = align >= 0, fuse != INT_MIN, handover != INT_MIN
    assert np.array_equal(a_has, f_has) and np.array_equal(a_has, h_has), (np.flatnonzero(a_has != f_has)[:8], np.flatnonzero(a_has != h_has)[:8])
    owner = lambda x: np.where(x >= 0, x, -1 - x.astype(np.int64))
    assert np.array_equal(owner(fuse)[a_has], align[a_has]) and np.array_equal(owner(handover)[a_has], align[a_has])
    assert np.array_equal(a_has, want), np.flatnonzero(a_has != want)[:8]
    # the owners themselves are the restatement's
    _, _, _, assoc, g = np_kf_align_sums(*D, R, t, **md)
    assert min(g.values()) > GUARD, g
    assert np.array_equal(align, assoc), (np.flatnonzero(align != assoc)[:8], align[align != assoc][:8], assoc[align != assoc][:8])


# ---- 2. one evaluation and one solve -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_one_evaluation_and_one_solve(B, scenes, cid):
    S = scenes(cid)
    ctx, mc, sr = S.ctx, S.mc, sr_of(S)
    snap, D, A = S.crafted()
    R, t = true_motion()
    used = assert_evaluation(B, ctx, mc, snap, D, R, t, f"{cid}: crafted motion", max_dist=sr)
    assert used >= 0.99 * len(A["prs4"]), (used, len(A["prs4"]))
    (Rg, tg), = seeded_guesses(1, 11, R, t)
    used_g = assert_evaluation(B, ctx, mc, snap, D, Rg, tg, f"{cid}: seeded guess", max_dist=sr)
    assert 12 <= used_g < used
    # the solve of test_solve_from_the_offsets, from the first offset; opts = None: the context's defaults, max_dist = search_range
    R0, t0 = offset_guess(*OFFSETS[0])
    ref = np_kf_align(*D, R0, t0, max_dist=sr)
    assert ref["guard"] > GUARD, ref["guard"]
    got, assoc = mc.keyframe_align(snap, None, R0, t0, want_assoc=True)
    e_np, e_dev, d = pose_err(ref["R"], ref["t"]), pose_err(got.R, got.t), pose_err(got.R, got.t, ref["R"], ref["t"])
    print(f"{cid}: used {used} / {used_g}; solve: err np {e_np:.3g} device {e_dev:.3g} |device - np| {d:.3g} used {got.used} of {got.candidates} "
          f"cond(H) {np.linalg.cond(ref['H']):.1f} guard {ref['guard']:.3g}")
    assert ref["status"] == 0 == got.status and got.iterations == 8 == ref["iterations"]
    assert got.used == ref["used"] and got.candidates == len(D[1]) and np.array_equal(assoc, ref["assoc"])
    assert e_np <= 1e-5
    assert DEV_VS_NP <= 0.1 * e_np
    assert d <= DEV_VS_NP
    S2, absS, used2, a2, _ = np_kf_align_sums(*D, np.array(got.R), np.array(got.t), max_dist=sr)
    assert used2 == got.used and np.array_equal(a2, assoc)
    assert (np.abs(pose_sums(got) - S2) <= (used2 + 64) * 2.0 ** -52 * absS).all()
    assert same_bytes(got, mc.keyframe_align(snap, None, R0, t0))


# ---- 3. distances the default never reaches -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,reach", [("C", 41), ("D", 128)])
def test_distances_the_default_range_never_reaches(B, scenes, cid, reach):
    """The gradient gate off, a fifth of the crafted keylines displaced by 15 px and one planted keyline per distance the field holds
    (context_cases.distance_case). The restatement shows keylines that are associated at max_dist = search_range and not at
    reach - 1: their cells lie at distance >= reach - past 40 in C, needing bit 7 of the key's distance field in D. Then max_dist
    over 0, 1, 40, reach - 1, search_range - 1 and search_range: assoc is exact at each, used never falls and grows above 40."""
    S = scenes(cid)
    ctx, mc, sr = S.ctx, S.mc, sr_of(S)
    far = int(S.cur[3][S.cur[2] >= 0].max())
    assert far >= (152 if cid == "D" else reach), far             # (152: the distance the issue's max_dist plant chose in D)
    case = distance_case(S.cam, S.kl, S.cur, room=len(S.base))
    snap, D = S.snapshot(craft_kf_keylines(S.base, case))
    R, t = true_motion()
    a_full = np_kf_align_sums(*D, R, t, min_cos=-1.0, max_dist=sr)[3]
    a_near = np_kf_align_sums(*D, R, t, min_cos=-1.0, max_dist=reach - 1)[3]
    beyond = (a_full >= 0) & (a_near < 0)
    planted_far = np.zeros(len(beyond), bool)                     # (the snapshot has the keyframe map's size: filtered keylines behind)
    planted_far[:len(case["plant_dist"])] = case["plant_dist"] >= reach
    print(f"{cid}: field reaches {far}; {int(beyond.sum())} keylines associated at distance >= {reach}, {int((beyond & planted_far).sum())} of them "
          f"planted there")
    assert beyond.sum() >= 1 and (beyond & planted_far).sum() >= 1
    assert np.array_equal(a_full[a_near >= 0], a_near[a_near >= 0])
    sweep = sorted({0, 1, 40, reach - 1, sr - 1, sr})
    used = [assert_evaluation(B, ctx, mc, snap, D, R, t, f"{cid}: max_dist {md}", min_cos=-1.0, max_dist=md) for md in sweep]
    print(f"{cid}: max_dist {sweep} -> used {used}")
    assert all(a <= b for a, b in zip(used, used[1:])) and used[0] > 0
    assert used[-1] > used[sweep.index(40)] and used[sweep.index(sr - 1)] > used[sweep.index(reach - 1)]


# ---- 4. many hypotheses --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_three_hypotheses_on_two_snapshots_of_unequal_size(B, scenes, cid):
    S = scenes(cid)
    ctx, mc, sr = S.ctx, S.mc, sr_of(S)
    big, D_big, A = S.crafted()
    # a smaller keyframe map: the same frame detected through a mask that lets the upper third of the pixels through
    rows, cols = ctx.rows, ctx.cols
    mask = np.zeros(rows * cols, np.uint8)
    mask[:rows * cols // 3] = 1
    ctx.set_detection_mask(mask.reshape(rows, cols))
    ms = ctx.detect_u8(frames_of(cid)[1], 0)
    ctx.set_detection_mask(None)
    n = ms.size()
    assert 64 < n < len(D_big[1]), (n, len(D_big[1]))
    base = ms.keylines()
    base["matches"] = 0
    ms.upload(craft_kf_keylines(base, A, min(n, len(A["prs4"]))))
    small = ms.keyframe_snapshot()
    small.add_normals(ms)
    S.snaps.append(small)
    D_small = (D_big[0], *small.download(), small.normals(), *S.cur)
    R, t = true_motion()
    g1, g2 = seeded_guesses(2, 12, R, t)
    items = [(big, D_big, R, t), (small, D_small, *g1), (big, D_big, *g2)]
    for max_iter in (0, 8):
        opts = B.default_kf_align_opts(ctx, max_iter=max_iter)
        assert opts.max_dist == sr
        res = mc.keyframe_align_many([B.kf_hypothesis(s, R0, t0) for s, _, R0, t0 in items], opts)
        assert [r.pose.candidates for r in res] == [len(D_big[1]), n, len(D_big[1])]
        for k, ((s, D, R0, t0), r) in enumerate(zip(items, res)):
            one = mc.keyframe_align(s, opts, R0, t0)
            assert bytes(r.pose) == bytes(one), (cid, max_iter, k, r.pose.status, one.status, r.pose.used, one.used)
            assert r.reserved == 0 and r.pose.used >= 12
            inl, used, g = np_inliers(*D, np.array(r.pose.R), np.array(r.pose.t), max_dist=sr)
            assert min(g.values()) > GUARD, (cid, max_iter, k, g)
            assert (r.pose.used, r.inliers) == (used, inl), (cid, max_iter, k, r.pose.used, used, r.inliers, inl)
    ms.release()


# ---- 5. fusion and hand-over ---------------------------------------------------------------------------------------------------------
def perturbed_keyframe(S, seed=1):
    """the crafted keyframe keylines with rho moved within sigma_rho (kf_fuse_ref.perturbed), as tests/test_keyframe_fuse_gpu.py has them"""
    from kf_align_ref import craft_against
    A = dict(craft_against(S.kl, S.cur[2], S.cur[3], seed, S.cam))
    A["prs4"], _ = perturbed(A, seed + 100)
    return craft_kf_keylines(S.base, A, min(len(A["prs4"]), len(S.base)))


@pytest.mark.parametrize("cid", IDS)
def test_fusion_bit_for_bit(B, scenes, cid):
    S = scenes(cid)
    ctx, mc, sr = S.ctx, S.mc, sr_of(S)
    snap, D = S.snapshot(perturbed_keyframe(S))
    R, t = true_motion()
    for what, kw in (("the context's reach", {}), ("no gradient test, tight gate", dict(min_cos=-1.0, gate_sigma=0.8, q_abs=0.02, pixel_sigma=0.5))):
        D = (D[0], *snap.download(), *D[3:])
        opts = B.default_kf_fuse_opts(ctx, **kw)
        assert opts.max_dist == sr
        ref = np_kf_fuse(*D, R, t, max_dist=sr, **kw)
        assert min(ref["guards"].values()) > GUARD, (cid, what, ref["guards"])
        hk, hp, hm, ha = B.kf_fuse_host(*D[0], sr, *D[1:], opts, R, t)
        got, assoc = snap.fuse_depth(mc, R, t, opts, want_assoc=True)
        prs4, mt = snap.download()
        print(f"{cid}, {what}: {fuse_counts(ref)}")
        for side, (cn, p, m, a) in (("hook", (hk, hp, hm, ha)), ("device", (got, prs4, mt, assoc))):
            assert fuse_counts(cn) == fuse_counts(ref), (cid, what, side, fuse_counts(cn), fuse_counts(ref))
            assert np.array_equal(a, ref["assoc"]), (cid, what, side, np.flatnonzero(a != ref["assoc"])[:8])
            assert p.tobytes() == ref["prs4"].tobytes(), (cid, what, side, np.flatnonzero((p != ref["prs4"]).any(1))[:8])
            assert np.array_equal(m, ref["matches"]), (cid, what, side)
        assert got.associated == got.fused + got.gated + got.flat and got.candidates == len(D[1])
        assert ref["fused"] > 0.5 * ref["candidates"], (cid, what, fuse_counts(ref))


@pytest.mark.parametrize("cid", IDS)
def test_handover_bit_for_bit_with_collisions(B, scenes, cid):
    S = scenes(cid)
    ctx, mc, sr = S.ctx, S.mc, sr_of(S)
    src, D = S.snapshot(perturbed_keyframe(S))
    R, t = true_motion()
    # the successor: a third detected map of the context takes its records by upload (the hand-over reads dst's buffers only)
    md = ctx.detect_u8(frames_of(cid)[0], 2 * TS)
    m = md.size()
    assert m > 500
    blank = np.zeros((m, 4), F32)
    blank[:, 2:] = (1.0, 1e9)
    prop = np_kf_handover(*D, blank, np.zeros(m, np.uint32), R, t, max_dist=sr)
    md.upload(successor_records(prop, m, 7, md.keylines()))
    dst = md.keyframe_snapshot()
    S.snaps.append(dst)
    for what, kw in (("the context's reach", {}), ("no gradient test, wide gate", dict(min_cos=-1.0, gate_sigma=30.0, q_abs=0.001))):
        dp, dm = dst.download()
        args = (*D, dp, dm)
        opts = B.default_kf_handover_opts(ctx, **kw)
        assert opts.max_dist == sr
        ref = np_kf_handover(*args, R, t, max_dist=sr, **kw)
        assert guard_min(ref) > GUARD, (cid, what, ref["guards"])
        losers = ref["associated"] - ref["out_of_range"] - ref["claimed"]
        print(f"{cid}, {what}: {handover_counts(ref)}, {losers} claimants lost their owner to another")
        assert losers >= 1                                       # the winner-per-owner rule runs on collisions
        assert what != "the context's reach" or (ref["adopted"] > 0.2 * ref["candidates"] and ref["kept"] > 0 and ref["conflicts"] > 0)
        hk, hp, hm, ha = B.kf_handover_host(*args[0], sr, *args[1:], opts, R, t)
        got, assoc = dst.handover_depth(src, mc, R, t, opts, want_assoc=True)
        prs4, mt = dst.download()
        for side, (cn, p, mm, a) in (("hook", (hk, hp, hm, ha)), ("device", (got, prs4, mt, assoc))):
            assert handover_counts(cn) == handover_counts(ref), (cid, what, side, handover_counts(cn), handover_counts(ref))
            assert np.array_equal(a, ref["assoc"]), (cid, what, side, np.flatnonzero(a != ref["assoc"])[:8])
            assert p.tobytes() == ref["prs4"].tobytes(), (cid, what, side, np.flatnonzero((p != ref["prs4"]).any(1))[:8])
            assert np.array_equal(mm, ref["matches"]), (cid, what, side)
        assert_identities(handover_counts(got))
        sp, sm = src.download()
        assert sp.tobytes() == D[1].tobytes() and sm.tobytes() == D[2].tobytes()          # src is never written
    md.release()


# ---- 6. defaults and refusals --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_defaults_and_refusals_follow_the_context(B, scenes, cid):
    """max_dist defaults to the context's search_range, search_range itself is accepted and search_range + 1 refused with -3 by all
    three entries - at 3 (B), 7, 100 and 255 (D)"""
    S = scenes(cid)
    ctx, mc, sr = S.ctx, S.mc, sr_of(S)
    assert sr == int(CONTEXTS[cid]["search_range"])
    assert B.default_kf_align_opts(ctx).max_dist == B.default_kf_fuse_opts(ctx).max_dist == B.default_kf_handover_opts(ctx).max_dist == sr
    snap, D, A = S.crafted()
    dst = mc.keyframe_snapshot()
    S.snaps.append(dst)
    R, t = true_motion()
    base = B.test_live_resources()
    calls = (("align", lambda md: mc.keyframe_align(snap, B.default_kf_align_opts(ctx, max_dist=md), R, t)),
             ("align_many", lambda md: mc.keyframe_align_many([B.kf_hypothesis(snap, R, t)], B.default_kf_align_opts(ctx, max_dist=md))),
             ("handover", lambda md: dst.handover_depth(snap, mc, R, t, B.default_kf_handover_opts(ctx, max_dist=md))),
             ("fuse", lambda md: snap.fuse_depth(mc, R, t, B.default_kf_fuse_opts(ctx, max_dist=md))))
    for name, call in calls:
        with pytest.raises(B.HipError) as e:
            call(sr + 1)
        assert "error -3:" in str(e.value) and "max_dist" in str(e.value), (cid, name, str(e.value))
    assert B.test_live_resources() == base                       # a refused call takes nothing
    for name, call in calls:
        call(sr)


# ---- 7. a batch lane -------------------------------------------------------------------------------------------------------------------
def test_a_batch_lane_aligns_its_maps_like_a_stand_alone_context(B, scenes):
    """A two-lane batch of row A: each lane's context detects the two frames itself and aligns its current map against a snapshot of
    its keyframe map. Keylines, field and every byte of the result equal the stand-alone context's."""
    S = scenes("A")
    snap, D, A = S.crafted()
    kf = craft_kf_keylines(S.base, A, min(len(A["prs4"]), len(S.base)))
    R, t = true_motion()
    R0, t0 = offset_guess(*OFFSETS[0])
    want0, assoc0 = S.mc.keyframe_align(snap, B.default_kf_align_opts(S.ctx, max_iter=0), R, t, want_assoc=True)
    want8, assoc8 = S.mc.keyframe_align(snap, None, R0, t0, want_assoc=True)
    assert want8.status == 0 and want0.used >= 0.99 * len(A["prs4"])
    frames = frames_of("A")
    bat = B.Batch(context_params(B, "A"), 2)
    for lane in bat.lanes:
        mk, mc = [lane.detect_u8(frames[1 + k], k * TS) for k in range(2)]
        assert mk.size() == S.mk.size() and mc.keylines().tobytes() == S.kl.tobytes()
        ids, dists = mc.distance_field()
        assert np.array_equal(ids.reshape(-1), S.cur[2]) and np.array_equal(dists.reshape(-1), S.cur[3])
        mk.upload(kf)
        ls = mk.keyframe_snapshot()
        ls.add_normals(mk)
        got0, a0 = mc.keyframe_align(ls, B.default_kf_align_opts(lane, max_iter=0), R, t, want_assoc=True)
        got8, a8 = mc.keyframe_align(ls, None, R0, t0, want_assoc=True)
        assert same_bytes(got0, want0) and np.array_equal(a0, assoc0)
        assert same_bytes(got8, want8) and np.array_equal(a8, assoc8)
        ls.release()
        mk.release()
        mc.release()
    bat.close()
