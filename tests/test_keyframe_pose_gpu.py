"""Keyframe snapshot and keyframe-to-current pose on the device: rebvio_hip_map_keyframe_snapshot / _kf_snapshot_download / _release
and rebvio_hip_map_keyframe_pose (k_kf_snapshot, k_kf_pose_sums, k_kf_pose_step). The contracts:
  - a snapshot holds pos_img, rho, sigma_rho and matches of its map as they were when it was taken, bit for bit, whatever happens to
    the map afterwards, and taking it changes nothing of the map;
  - the 28 sums of one evaluation equal np_kf_pose_sums (tests/kf_pose_ref.py) on the data downloaded just before, each within
    (used + 64) * 2^-52 * sum |term| - per-term arithmetic is IEEE fp64 in the same order on both sides, which leaves at most
    used - 1 roundings of 2^-53 relative to sum |term| per side; the 64 is slack for sqrt and the final adds - `used` and
    `candidates` equal as integers, and two calls in a row equal in every output byte;
  - every skip rule of the definition drops exactly the keylines planted for it;
  - the solve recovers the crafted motion as well as the restatement does, follows it through outliers, and reports its statuses.
All maps are 160x120 with keylines_max <= 800 unless a case says otherwise."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import params_for
from kf_pose_ref import craft_arrays, craft_keylines, np_kf_pose, np_kf_pose_sums, off_guess, pose_err, pose_sums
from support import B, refusal_scene  # noqa: F401
from support import DEAD_MAP, DEAD_SNAPSHOT, assert_refused, foreign_snapshot
from support import F32, TS, assert_keylines_equal, enlarged_stream, np_kf_matches, rec, same_records, ulp_down, ulp_up, vision_only_fusion

pytestmark = pytest.mark.gpu

W, H, NF = 160, 120, 10
KW = dict(keylines_ref=600, keylines_max=800, global_min_matches_threshold=50)
# |device - numpy| over R and t on the clean crafted cases (test_solve_on_clean_data) - measured maximum on an MI355X: 1.53e-16 (device
# sin / cos and the Cholesky order differ from numpy's by a few ulp, amplified by cond(H) of 20..55); the bound is 100 x that. It has
# to stay <= 0.1 x the smallest err(np_kf_pose) of those cases (2.66e-9), which the test asserts as a condition. (The six poses along
# the synthetic stream, held to the same bound, measured 3.3e-16 at most.)
DEV_VS_NP = 1.53e-14


@functools.lru_cache(maxsize=None)
def stream():
    from rebvio_amd import synth
    return synth.render_stream(W, H, NF)


def sized_maps(B, n, count=2):
    """(context, maps) with exactly n keylines each: keylines_max = n truncates the frames' keylines (n = 0: blank frames)"""
    frames, cam = stream()
    if n == 0:
        ctx = B.Context(params_for(B, cam, **KW))
        maps = [ctx.detect_u8(np.full((H, W), 128, np.uint8), k * TS) for k in range(count)]
    else:
        ctx = B.Context(params_for(B, cam, keylines_ref=max(1, n - 1), keylines_max=n, global_min_matches_threshold=1))
        maps = [ctx.detect_u8(frames[1 + k], k * TS) for k in range(count)]
    assert all(m.size() == n for m in maps), (n, [m.size() for m in maps])
    return ctx, maps


def crafted_pair(B, n, seed=None, **craft):
    """(context, keyframe map, current map, snapshot, arrays): craft_arrays uploaded into two maps of n keylines, the keyframe
    snapshotted"""
    ctx, (mk, mc) = sized_maps(B, n)
    A = craft_arrays(n, n if seed is None else seed, ctx.p.fm, W, H, **craft)
    kf, cur = craft_keylines(mk.keylines(), mc.keylines(), A)
    mk.upload(kf)
    mc.upload(cur)
    return ctx, mk, mc, mk.keyframe_snapshot(), A


def downloaded(ctx, snap, m):
    """what the restatement is given: the snapshot, the map's keylines and its correspondences, all downloaded just before"""
    prs4, mt = snap.download()
    kl = m.keylines()
    recs, _ = np_kf_matches(kl, len(prs4))
    return (ctx.p.fm, prs4, mt, kl["pos_img"], kl["gradient"], recs)


def assert_sums(got, data, R, t, what, **kw):
    S, absS, used = np_kf_pose_sums(*data, R, t, **kw)
    assert got.candidates == len(data[5]) and got.used == used, (what, got.candidates, len(data[5]), got.used, used)
    d = np.abs(pose_sums(got) - S)
    bound = (used + 64) * 2.0 ** -52 * absS
    assert (d <= bound).all(), (what, np.flatnonzero(d > bound), d[d > bound], bound[d > bound])
    return used


def same_bytes(a, b):
    return bytes(a) == bytes(b)


def random_guess(seed):
    from support import rodrigues
    rng = np.random.default_rng(seed)
    return rodrigues(rng.uniform(-0.1, 0.1, 3)), rng.uniform(-0.2, 0.2, 3)


# ---- 1. the snapshot -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 257])
def test_snapshot_equals_the_map_and_changes_nothing(B, n):
    """the wave and workgroup edges of k_kf_snapshot"""
    ctx, (m, _) = sized_maps(B, n)
    before = m.keylines()
    snap = m.keyframe_snapshot()
    prs4, mt = snap.download()
    assert prs4.shape == (n, 4) and mt.shape == (n,)
    assert prs4[:, :2].tobytes() == np.ascontiguousarray(before["pos_img"]).tobytes()
    assert prs4[:, 2].tobytes() == before["rho"].tobytes() and prs4[:, 3].tobytes() == before["sigma_rho"].tobytes()
    assert np.array_equal(mt, before["matches"])
    assert_keylines_equal(before, m.keylines(), f"n = {n}")
    snap.release()
    ctx.close()


def test_download_with_a_cap_below_the_size(B):
    ctx, (m, _) = sized_maps(B, 257)
    kl = m.keylines()
    snap = m.keyframe_snapshot()
    L = B.lib()
    prs, mt, n = np.full((20, 4), -7.0, F32), np.full(20, 9, np.uint32), C.c_int()
    assert L.rebvio_hip_kf_snapshot_download(snap.h, prs.ctypes.data_as(C.POINTER(C.c_float)), mt.ctypes.data_as(C.POINTER(C.c_uint)), 10, C.byref(n)) == 0
    assert n.value == 257 and np.array_equal(prs[:10, :2], kl["pos_img"][:10]) and (prs[10:] == -7.0).all() and (mt[10:] == 9).all()
    snap.release()
    ctx.close()


def test_snapshot_survives_its_map_being_tracked_as_an_old_map(B):
    frames, cam = stream()
    ctx = B.Context(params_for(B, cam, **KW))
    maps = [ctx.detect_u8(frames[k], k * TS) for k in range(4)]
    assert ctx.track_pair(maps[0], maps[1]).status == 0
    before = maps[1].keylines()
    maps[1].mark_keyframe()
    snap = maps[1].keyframe_snapshot()
    for k in (2, 3):    # map 1 as the old map of two pairs: rotated in place twice
        assert ctx.track_pair(maps[1], maps[k]).status == 0
    after = maps[1].keylines()
    assert (before["pos_img"] != after["pos_img"]).any(1).sum() > 100
    prs4, mt = snap.download()
    assert prs4[:, :2].tobytes() == np.ascontiguousarray(before["pos_img"]).tobytes()
    assert prs4[:, 2].tobytes() == before["rho"].tobytes() and prs4[:, 3].tobytes() == before["sigma_rho"].tobytes()
    assert np.array_equal(mt, before["matches"])
    snap.release()
    ctx.close()


def test_refusals_and_handles_that_outlive_their_context(B):
    frames, cam = stream()
    live = B.test_live_resources()
    ctx, other = B.Context(params_for(B, cam, **KW)), B.Context(params_for(B, cam, **KW))
    maps = [ctx.detect_u8(frames[k], k * TS) for k in range(3)]
    foreign = other.detect_u8(frames[0], 0)
    L = B.lib()
    err = lambda: L.rebvio_hip_last_error().decode()
    h, n, out = C.c_void_p(), C.c_int(), B.KfPose()
    assert L.rebvio_hip_map_keyframe_snapshot(None, maps[0].h, C.byref(h)) == -3 and "null" in err()
    assert L.rebvio_hip_map_keyframe_snapshot(ctx.h, None, C.byref(h)) == -3 and "null" in err()
    assert L.rebvio_hip_map_keyframe_snapshot(ctx.h, maps[0].h, None) == -3 and "null" in err()
    assert L.rebvio_hip_map_keyframe_snapshot(ctx.h, foreign.h, C.byref(h)) == -3 and "another context" in err() and not h.value
    base = B.test_live_resources()
    snap, fsnap = maps[0].keyframe_snapshot(), foreign.keyframe_snapshot()
    assert B.test_live_resources() == base + 2                  # one buffer per snapshot
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint)
    assert L.rebvio_hip_kf_snapshot_download(snap.h, None, None, 0, None) == -3 and "null" in err()
    assert L.rebvio_hip_kf_snapshot_download(snap.h, None, None, -1, C.byref(n)) == -3 and "cap" in err()
    assert L.rebvio_hip_kf_snapshot_download(snap.h, None, None, 4, C.byref(n)) == -3 and "cap" in err()
    # the pose entry: every refusal before the device is touched
    assert L.rebvio_hip_map_keyframe_pose(None, snap.h, None, None, None, C.byref(out)) == -3 and "null" in err()
    assert L.rebvio_hip_map_keyframe_pose(maps[0].h, None, None, None, None, C.byref(out)) == -3 and "null" in err()
    assert L.rebvio_hip_map_keyframe_pose(maps[0].h, snap.h, None, None, None, None) == -3 and "null" in err()
    assert L.rebvio_hip_map_keyframe_pose(maps[0].h, fsnap.h, None, None, None, C.byref(out)) == -3 and "another context" in err()
    nan_R = np.eye(3)
    nan_R[2, 0] = np.nan
    for kw, word in ((dict(R0=nan_R), "non-finite"), (dict(t0=[0.0, 0.0, -np.inf]), "non-finite"),
                     (dict(opts=B.default_kf_pose_opts(huber_px=0.0)), "huber_px"), (dict(opts=B.default_kf_pose_opts(huber_px=float("nan"))), "huber_px"),
                     (dict(opts=B.default_kf_pose_opts(max_iter=33)), "max_iter"), (dict(opts=B.default_kf_pose_opts(max_iter=-1)), "max_iter"),
                     (dict(opts=B.default_kf_pose_opts(min_used=-1)), "min_used"),
                     (dict(opts=B.default_kf_pose_opts(kf_filter=dict(rho_min=-1.0))), "rho_min"),
                     (dict(opts=B.default_kf_pose_opts(kf_filter=dict(max_rel_sigma=float("nan")))), "NaN")):
        with pytest.raises(B.HipError) as e:
            maps[0].keyframe_pose(snap, **kw)
        assert "error -3:" in str(e.value) and word in str(e.value), (kw, str(e.value))
    # a map promised to R_prior_next is rotated for the next pair: no snapshot, no pose (-7) until the next _begin has run
    c, s = F32(np.cos(0.01)), F32(np.sin(0.01))
    Rn = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], F32)
    mid = ctx.track_pair_begin(maps[0], maps[1])
    ctx.track_pair_finish_async(maps[0], maps[1], *vision_only_fusion(mid), R_prior_next=Rn)
    assert ctx.track_pair_result()[3] == 0
    held = B.test_live_resources()
    for call in (maps[1].keyframe_snapshot, lambda: maps[1].keyframe_pose(snap)):
        with pytest.raises(B.HipError) as e:
            call()
        assert "error -7:" in str(e.value) and "R_prior_next" in str(e.value), str(e.value)
    assert B.test_live_resources() == held                      # a refused call takes nothing
    mid = ctx.track_pair_begin(maps[1], maps[2], R_prior=Rn)
    ctx.track_pair_finish_async(maps[1], maps[2], *vision_only_fusion(mid))
    assert ctx.track_pair_result()[3] == 0
    late = maps[2].keyframe_snapshot()
    assert late.download()[0].shape == (maps[2].size(), 4)
    late.release()
    snap.release()                                              # a release while the context lives gives the buffer back at once
    snap = maps[0].keyframe_snapshot()
    gone = C.c_void_p(ctx.h.value)
    ctx.close()
    assert L.rebvio_hip_map_keyframe_snapshot(gone, maps[0].h, C.byref(h)) == -10 and "destroyed" in err()
    assert L.rebvio_hip_kf_snapshot_download(snap.h, None, None, 0, C.byref(n)) == -10 and "destroyed" in err()
    assert L.rebvio_hip_map_keyframe_pose(maps[0].h, snap.h, None, None, None, C.byref(out)) == -10 and "destroyed" in err()
    assert L.rebvio_hip_map_keyframe_pose(foreign.h, snap.h, None, None, None, C.byref(out)) == -10 and "destroyed" in err()
    snap.release()                                              # after close(): still safe
    fsnap.release()
    other.close()
    for m in maps + [foreign]:
        m.release()
    assert B.test_live_resources() == live


def test_live_resources_return_to_their_start(B):
    live = B.test_live_resources()
    ctx, mk, mc, snap, _ = crafted_pair(B, 64)
    base = B.test_live_resources()
    assert mc.keyframe_pose(snap).status == 0
    assert B.test_live_resources() == base + 3                  # correspondence table, records, pose scratch: on first use ...
    mc.keyframe_pose(snap)
    assert B.test_live_resources() == base + 3                  # ... and kept
    snap.release()
    assert B.test_live_resources() == base + 2                  # (base counted the snapshot)
    kept = mk.keyframe_snapshot()
    ctx.close()
    kept.release()
    assert B.test_live_resources() == live


# ---- 2. the sums ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 800])
def test_sums_on_crafted_maps(B, n):
    """the wave edge, the workgroup edge and several partials; at the identity and at a random guess"""
    ctx, mk, mc, snap, _ = crafted_pair(B, n)
    data = downloaded(ctx, snap, mc)
    opts = B.default_kf_pose_opts(max_iter=0)
    for R0, t0 in ((None, None), random_guess(n)):
        got = mc.keyframe_pose(snap, opts, R0, t0)
        R, t = (np.eye(3), np.zeros(3)) if R0 is None else (R0, t0)
        assert assert_sums(got, data, R, t, f"n {n}") == n
        assert (got.status, got.iterations) == (3 if n < 12 else 0, 0)
        assert np.array_equal(np.array(got.R), R.reshape(9)) and np.array_equal(np.array(got.t), t)
        assert same_bytes(got, mc.keyframe_pose(snap, opts, R0, t0))           # two calls in a row
    snap.release()
    ctx.close()


def test_sums_on_the_synthetic_stream(B):
    """four pairs behind a marked and snapshotted frame 2: real depths, several claimants per slot, keylines the filter drops"""
    frames, cam = stream()
    ctx = B.Context(params_for(B, cam, **KW))
    maps = [ctx.detect_u8(frames[k], k * TS) for k in range(7)]
    for k in range(6):
        assert ctx.track_pair(maps[k], maps[k + 1]).status == 0
        if k == 1:
            maps[2].mark_keyframe()
            snap = maps[2].keyframe_snapshot()
    m = maps[6]
    data = downloaded(ctx, snap, m)
    opts = B.default_kf_pose_opts(max_iter=0)
    for R0, t0 in ((None, None), random_guess(4)):
        got = m.keyframe_pose(snap, opts, R0, t0)
        R, t = (np.eye(3), np.zeros(3)) if R0 is None else (R0, t0)
        used = assert_sums(got, data, R, t, "stream")
        print("candidates", got.candidates, "used", used)
        assert 64 < used < got.candidates
        assert same_bytes(got, m.keyframe_pose(snap, opts, R0, t0))
    snap.release()
    ctx.close()


def test_sums_over_more_than_128_partials(B):
    """keylines_max = 65 536 on a 2304 x 1900 frame: a keyframe of more than 32 768 keylines, i.e. more than 128 workgroup partials
    added up by k_kf_pose_step"""
    Wb, Hb = 2304, 1900
    frames, cam = enlarged_stream(Wb, Hb, 3)
    ctx = B.Context(B.default_params(Hb, Wb, fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=60000, keylines_max=65536))
    maps = sorted((ctx.detect_u8(frames[i], i * 50000) for i in range(3)), key=lambda x: -x.size())
    mk, mc = maps[0], maps[1]
    n = min(mk.size(), mc.size())
    print("keyframe", mk.size(), "current", mc.size())
    assert n > 32768
    A = craft_arrays(n, 11, ctx.p.fm, Wb, Hb)
    kf, cur = craft_keylines(mk.keylines(), mc.keylines(), A)
    mk.upload(kf)
    mc.upload(cur)
    snap = mk.keyframe_snapshot()
    data = downloaded(ctx, snap, mc)
    R0, t0 = random_guess(7)
    got = mc.keyframe_pose(snap, B.default_kf_pose_opts(max_iter=0), R0, t0)
    assert assert_sums(got, data, R0, t0, "large") > 32768
    assert same_bytes(got, mc.keyframe_pose(snap, B.default_kf_pose_opts(max_iter=0), R0, t0))
    snap.release()
    ctx.close()


# ---- 3. every skip rule, one keyline each ----------------------------------------------------------------------------------------
def test_every_skip_rule_drops_exactly_its_keyline(B):
    n = 257
    ctx, (mk, mc) = sized_maps(B, n)
    A = craft_arrays(n, 31, ctx.p.fm, W, H)
    kf0, cur0 = craft_keylines(mk.keylines(), mc.keylines(), A)
    flt = dict(min_matches=3, max_rel_sigma=0.25, rho_min=0.125, rho_max=4.0)
    opts = B.default_kf_pose_opts(max_iter=0, kf_filter=flt)
    nflt = (3, 0.25, 0.125, 4.0)
    R0, t0 = off_guess(5)

    def run(kf, cur, R=R0, t=t0):
        mk.upload(kf)
        mc.upload(cur)
        snap = mk.keyframe_snapshot()
        data = downloaded(ctx, snap, mc)
        got = mc.keyframe_pose(snap, opts, R, t)
        used = assert_sums(got, data, R, t, "skip", flt=nflt)
        snap.release()
        return used, got

    assert run(kf0, cur0)[0] == n
    # keyframe side, one keyline each: matches below the filter, rho one ulp outside each bound (and exactly on it: kept), sigma_rho one
    # ulp above max_rel_sigma * rho (and exactly on it: kept), rho NaN
    kf = kf0.copy()
    kf["matches"][3] = 2
    kf["rho"][10], kf["sigma_rho"][10] = ulp_down(0.125), 0.0
    kf["rho"][11], kf["sigma_rho"][11] = F32(0.125), 0.0
    kf["rho"][20], kf["sigma_rho"][20] = ulp_up(4.0), 0.0
    kf["rho"][21], kf["sigma_rho"][21] = F32(4.0), 0.0
    kf["sigma_rho"][64] = ulp_up(F32(0.25) * kf["rho"][64])
    kf["sigma_rho"][65] = F32(0.25) * kf["rho"][65]
    kf["rho"][128] = np.nan
    assert run(kf, cur0)[0] == n - 5
    # current side: a zero, a NaN and an infinite gradient
    cur = cur0.copy()
    cur["gradient"][7] = (0.0, 0.0)
    cur["gradient"][63] = (np.nan, 1.0)
    cur["gradient"][256] = (1.0, np.inf)
    used, got = run(kf0, cur)
    assert used == n - 3 and np.isfinite(np.frombuffer(bytes(got), np.float64, 55)).all()
    # Y.z <= 0 through a guess with a large negative t.z: Y.z = Z.z + rho * t.z, Z.z within a few per cent of 1: rho > 0.6 goes, < 0.4 stays
    tz = np.array([0.0, 0.0, -2.0])
    want = int((1.0 + kf0["rho"].astype(np.float64) * -2.0 > 0.2).sum())
    used, _ = run(kf0, cur0, np.eye(3), tz)
    assert 0 < used < n and abs(used - want) <= 0.1 * n, (used, want)
    # ids: -1, kf_size and INT_MAX are no candidates; several claimants on one slot: only the winner (smallest sigma_rho) counts
    cur = cur0.copy()
    cur["match_id_keyframe"][[5, 70, 200]] = (-1, n, 2 ** 31 - 1)
    cur["match_id_keyframe"][[30, 31, 32]] = 30
    cur["sigma_rho"][[30, 31, 32]] = (0.3, 0.2, 0.25)          # keyline 31 wins slot 30; slots 31 and 32 are empty
    used, got = run(kf0, cur)
    assert used == n - 3 - 2 and got.candidates == n - 5
    ctx.close()


# ---- 4. the solve on clean crafted data ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [12, 64, 257, 800])
def test_solve_on_clean_data(B, n):
    ctx, mk, mc, snap, A = crafted_pair(B, n)
    data = downloaded(ctx, snap, mc)
    for R0, t0 in ((None, None), off_guess(n)):
        ref = np_kf_pose(*data, R0, t0)
        got = mc.keyframe_pose(snap, None, R0, t0)
        e_np, e_dev, d = pose_err(ref["R"], ref["t"]), pose_err(got.R, got.t), pose_err(got.R, got.t, ref["R"], ref["t"])
        print(f"n {n}: err np {e_np:.3g} dev {e_dev:.3g} |dev - np| {d:.3g} cond(H) {np.linalg.cond(ref['H']):.1f}")
        assert got.status == 0 == ref["status"] and got.iterations == 8 and got.used == n == got.candidates
        assert e_np <= 1e-6 and e_dev <= 2 * e_np
        assert DEV_VS_NP <= 0.1 * e_np
        assert d <= DEV_VS_NP
        assert_sums(got, data, np.array(got.R), np.array(got.t), "at the returned pose")
        assert same_bytes(got, mc.keyframe_pose(snap, None, R0, t0))
    snap.release()
    ctx.close()


# ---- 5. outliers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [800, 257])
def test_solve_with_outliers(B, n):
    """20 % of the current keylines displaced by +-15 px along their normal"""
    ctx, mk, mc, snap, A = crafted_pair(B, n, outliers=0.2)
    data = downloaded(ctx, snap, mc)
    ref, got = np_kf_pose(*data), mc.keyframe_pose(snap)
    ref_ls, got_ls = np_kf_pose(*data, huber=1e9), mc.keyframe_pose(snap, B.default_kf_pose_opts(huber_px=1e9))
    e_np, e_dev, e_np_ls, e_dev_ls = pose_err(ref["R"], ref["t"]), pose_err(got.R, got.t), pose_err(ref_ls["R"], ref_ls["t"]), pose_err(got_ls.R, got_ls.t)
    print(f"n {n}: err np huber {e_np:.3g} ls {e_np_ls:.3g}; dev huber {e_dev:.3g} ls {e_dev_ls:.3g}")
    assert got.status == 0 == got_ls.status
    assert e_np <= 1e-2 and e_dev <= 2 * e_np
    assert e_np_ls > e_np and e_dev_ls > e_np                    # plain least squares is worse: the weights are applied ...
    assert pose_err(got_ls.R, got_ls.t, ref_ls["R"], ref_ls["t"]) <= 1e-9   # ... and the device follows the restatement there
    snap.release()
    ctx.close()


# ---- 6. statuses ---------------------------------------------------------------------------------------------------------------------
def test_statuses(B):
    R0, t0 = off_guess(3)
    # used < min_used: status 3, pose = guess, the sums of the guess still returned
    ctx, mk, mc, snap, _ = crafted_pair(B, 11)
    data = downloaded(ctx, snap, mc)
    got = mc.keyframe_pose(snap, None, R0, t0)
    assert (got.status, got.iterations, got.used, got.candidates) == (3, 0, 11, 11)
    assert np.array_equal(np.array(got.R), R0.reshape(9)) and np.array_equal(np.array(got.t), t0)
    assert_sums(got, data, R0, t0, "status 3")
    assert mc.keyframe_pose(snap, B.default_kf_pose_opts(min_used=11), R0, t0).status == 0
    snap.release()
    ctx.close()
    # all gradients parallel (along x: J[1] == 0 in every term, so H(1, 1) == 0 exactly): status 2, pose = guess, no NaN anywhere
    ctx, mk, mc, snap, _ = crafted_pair(B, 64, parallel=True)
    data = downloaded(ctx, snap, mc)
    got = mc.keyframe_pose(snap, None, R0, t0)
    assert np_kf_pose(*data, R0, t0)["status"] == 2
    assert (got.status, got.iterations, got.used) == (2, 0, 64)
    assert np.array_equal(np.array(got.R), R0.reshape(9)) and np.array_equal(np.array(got.t), t0)
    assert np.isfinite(np.frombuffer(bytes(got), np.float64, 55)).all()
    assert_sums(got, data, R0, t0, "status 2")
    snap.release()
    ctx.close()


def test_an_empty_keyframe_launches_nothing(B):
    ctx, (mk, mc) = sized_maps(B, 0)
    snap = mk.keyframe_snapshot()
    assert snap.download()[0].shape == (0, 4)                    # (fetches the size: the one copy the entry may still need)
    ctx.profile_reset()
    ctx.profile(True)
    R0, t0 = off_guess(1)
    got = mc.keyframe_pose(snap, None, R0, t0)
    launches = {name: calls for name, (_, calls) in ctx.profile_read().items() if calls}
    ctx.profile(False)
    assert launches == {}, launches
    assert (got.status, got.candidates, got.used, got.iterations) == (3, 0, 0, 0)
    assert np.array_equal(np.array(got.R), R0.reshape(9)) and np.array_equal(np.array(got.t), t0)
    assert not np.array(got.H).any() and not np.array(got.g).any() and got.cost == 0.0
    snap.release()
    ctx.close()


def test_the_entry_launches_what_it_documents(B):
    """three kernels of the correspondences, then max_iter + 1 evaluations of two kernels each"""
    ctx, mk, mc, snap, _ = crafted_pair(B, 65)
    snap.download()
    ctx.profile_reset()
    ctx.profile(True)
    mc.keyframe_pose(snap, B.default_kf_pose_opts(max_iter=5))
    launches = {name: calls for name, (_, calls) in ctx.profile_read().items() if calls}
    ctx.profile(False)
    assert launches == dict(k_kf_claim=1, k_kf_count=1, k_kf_emit=1, k_kf_pose_sums=6, k_kf_pose_step=6), launches
    snap.release()
    ctx.close()


# ---- 7. the real stream --------------------------------------------------------------------------------------------------------------
def test_pose_along_the_synthetic_stream_and_nothing_disturbed(B):
    """snapshot at frame 2, six pairs, the pose after each pair warm-started from the previous one: every call status 0 and within
    DEV_VS_NP of the restatement on the downloaded data; the pair records and the final keylines equal a run without the feature"""
    frames, cam = stream()

    def run(with_pose):
        ctx = B.Context(params_for(B, cam, **KW))
        maps = [ctx.detect_u8(frames[k], k * TS) for k in range(9)]
        recs, snap, R, t = [], None, None, None
        for k in range(8):
            out = ctx.track_pair(maps[k], maps[k + 1])
            recs.append(rec(out, maps[k + 1].size()))
            if k == 1:
                maps[2].mark_keyframe()          # (marked in both runs: the ids are part of what is compared)
                if with_pose:
                    snap = maps[2].keyframe_snapshot()
            if k >= 2 and with_pose:
                data = downloaded(ctx, snap, maps[k + 1])
                got = maps[k + 1].keyframe_pose(snap, None, R, t)
                ref = np_kf_pose(*data, R, t)
                d = pose_err(got.R, got.t, ref["R"], ref["t"])
                print(f"pair {k}: candidates {got.candidates} used {got.used} status {got.status} |t| {np.linalg.norm(got.t):.4f} "
                      f"cost {got.cost:.1f} |dev - np| {d:.3g}")
                assert got.status == 0 == ref["status"] and got.iterations == 8
                assert d <= DEV_VS_NP
                R, t = np.array(got.R), np.array(got.t)
        final = maps[8].keylines()
        if snap:
            snap.release()
        ctx.close()
        return recs, final

    plain, kl_plain = run(False)
    posed, kl_posed = run(True)
    same_records(plain, posed, "with and without snapshot and pose calls")
    assert_keylines_equal(kl_plain, kl_posed, "final keylines")


# ---- the refusal table: every shared refusal with its code and whole text; which one wins when several apply ------

POSE = "map_keyframe_pose"
REFUSED = {
    "destroyed map": (lambda s: s.dm.keyframe_pose(s.dsnap), -10, DEAD_MAP),
    "destroyed snapshot": (lambda s: s.m.keyframe_pose(s.dsnap), -10, DEAD_SNAPSHOT),
    "foreign snapshot": (lambda s: s.m.keyframe_pose(s.fsnap), -3, foreign_snapshot(POSE)),
    "R0 not finite": (lambda s: s.m.keyframe_pose(s.snap, None, s.nan_R, s.t), -3, f"{POSE}: non-finite R0 or t0"),
    "t0 not finite": (lambda s: s.m.keyframe_pose(s.snap, None, None, s.inf_t), -3, f"{POSE}: non-finite R0 or t0"),
    "wins: an option over a guess": (lambda s: s.m.keyframe_pose(s.snap, s.B.default_kf_pose_opts(huber_px=0.0), s.nan_R), -3,
                                     f"{POSE}: huber_px must be > 0"),
    "wins: a guess over a destroyed map": (lambda s: s.dm.keyframe_pose(s.fsnap, None, s.nan_R), -3, f"{POSE}: non-finite R0 or t0"),
    "wins: a destroyed map over a foreign snapshot": (lambda s: s.dm.keyframe_pose(s.snap), -10, DEAD_MAP),
}

@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusal_table(refusal_scene, case):
    """every refusal of the table with its return code and its whole rebvio_hip_last_error text; nothing is allocated"""
    assert_refused(refusal_scene, *REFUSED[case])
