"""Snapshot normals and the alignment of a snapshot through a map's distance field on the device: rebvio_hip_kf_snapshot_add_normals /
_download_normals and rebvio_hip_map_keyframe_align (k_kf_snapshot_normals, k_kf_align_sums, k_kf_pose_step). The contracts:
  - the normals are gradient / gradient_norm of the map's download, bit for bit, zeros behind the smaller of the two sizes;
  - one evaluation associates every keyframe keyline with the keyline np_kf_align_sums (tests/kf_align_ref.py) associates it with, on
    the snapshot, keylines and distance field downloaded just before, and its 28 sums are within (used + 64) * 2^-52 * sum |term| of
    the restatement's (the bound of tests/test_keyframe_pose_gpu.py: per-term arithmetic is IEEE fp64 in the same order on both sides);
    two calls in a row are equal in every output byte;
  - every skip rule of the definition that can be planted on a detected map drops exactly the keyline planted for it (the owner's unit
    is detection's and cannot be planted: that rule is covered on the host, tests/test_keyframe_align.py, through the same source);
  - the solve follows the restatement from guesses 0.005 and 0.02 rad off the truth, through displaced keylines, and reports its statuses;
  - nothing of tracking is disturbed, and a map whose chain is gone (rebvio_hip_reset_state) is aligned again.
A comparison of associations or of an iterated solve is valid only while no term of the restatement comes within GUARD of a cell edge,
the gate or the Huber switch at any iterate; every comparison asserts that first. The keyframe keylines are crafted against the
current map (craft_against), uploaded into another map of the same context and snapshotted; the current map is a detected one.
All maps are 160x120 with keylines_max <= 1601 unless a case says otherwise."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import params_for
from kf_align_ref import (DEV_VS_NP, GUARD, OFFSETS, assert_evaluation, cam_of, craft_against, craft_kf_keylines, current_data, data_of, np_kf_align,
                          np_kf_align_sums, offset_guess, same_bytes, unit_of)
from kf_pose_ref import pose_err, pose_sums, true_motion
from support import B, refusal_scene  # noqa: F401
from support import DEAD_MAP, DEAD_SNAPSHOT, assert_refused, foreign_snapshot, no_field
from support import F32, TS, assert_keylines_equal, enlarged_stream, rec, rodrigues, same_records, vision_only_fusion

pytestmark = pytest.mark.gpu

W, H, NF = 160, 120, 10
KW_FULL = dict(keylines_ref=1200, keylines_max=1601, global_min_matches_threshold=1)
KW_STREAM = dict(keylines_ref=600, keylines_max=800, global_min_matches_threshold=50)      # the stream of the pose tests: every pair tracks


@functools.lru_cache(maxsize=None)
def stream():
    from rebvio_amd import synth
    return synth.render_stream(W, H, NF)


def sized_maps(B, n, count=2):
    """(context, maps) with exactly n keylines each: keylines_max = n truncates the frames' keylines (n = 0: blank frames)"""
    frames, cam = stream()
    if n == 0:
        ctx = B.Context(params_for(B, cam, **KW_STREAM))
        maps = [ctx.detect_u8(np.full((H, W), 128, np.uint8), k * TS) for k in range(count)]
    else:
        ctx = B.Context(params_for(B, cam, keylines_ref=max(1, n - 1), keylines_max=n, global_min_matches_threshold=1))
        maps = [ctx.detect_u8(frames[1 + k], k * TS) for k in range(count)]
    assert all(m.size() == n for m in maps), (n, [m.size() for m in maps])
    return ctx, maps


def snapshot_of(mk, kf_keylines):
    mk.upload(kf_keylines)
    snap = mk.keyframe_snapshot()
    snap.add_normals(mk)
    return snap


def crafted_scene(B, n=None, seed=1, displaced=0.0):
    """(context, keyframe map, current map, snapshot with normals, restatement data, crafted arrays). n: both maps hold exactly n
    keylines; None: the frames' own keylines under KW_FULL. Keyframe keylines behind the crafted ones are filtered out (matches 0)."""
    if n is None:
        frames, cam = stream()
        ctx = B.Context(params_for(B, cam, **KW_FULL))
        mk, mc = [ctx.detect_u8(frames[1 + k], k * TS) for k in range(2)]
    else:
        ctx, (mk, mc) = sized_maps(B, n)
    kl, cur = current_data(mc)
    A = craft_against(kl, cur[2], cur[3], seed, cam_of(ctx), displaced)
    base = mk.keylines()
    base["matches"] = 0
    snap = snapshot_of(mk, craft_kf_keylines(base, A, min(len(A["prs4"]), len(base))))
    return ctx, mk, mc, snap, data_of(ctx, snap, cur), A


def random_guess(seed):
    """a guess within 0.01 rad / 0.04 units of the crafted motion, so that a good share of the terms is used"""
    rng = np.random.default_rng(seed)
    R, t = true_motion()
    return rodrigues(rng.uniform(-0.01, 0.01, 3)) @ R, t + rng.uniform(-0.04, 0.04, 3)


# ---- 1. the normals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 257])
def test_normals_equal_gradient_over_norm_bit_for_bit(B, n):
    """the wave and workgroup edges of k_kf_snapshot_normals"""
    ctx, (m, _) = sized_maps(B, n)
    kl = m.keylines()
    snap = m.keyframe_snapshot()
    with pytest.raises(B.HipError, match="error -7:.*no normals"):
        snap.normals()
    snap.add_normals(m)
    got = snap.normals()
    assert got.shape == (n, 2) and got.tobytes() == unit_of(kl).tobytes()
    assert n == 0 or (np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1) < 1e-6).all()
    assert_keylines_equal(kl, m.keylines(), f"n = {n}")          # nothing of the map is written
    snap.add_normals(m)                                          # a second call overwrites
    assert snap.normals().tobytes() == got.tobytes()
    snap.release()
    ctx.close()


def test_normals_of_maps_of_other_sizes_and_zero_norms(B):
    frames, cam = stream()
    ctx = B.Context(params_for(B, cam, **KW_FULL))
    blank = ctx.detect_u8(np.full((H, W), 128, np.uint8), 0)
    m1, m2 = ctx.detect_u8(frames[1], TS), ctx.detect_u8(frames[2], 2 * TS)
    n1, n2 = m1.size(), m2.size()
    assert blank.size() == 0 and n1 > 257 and n2 > 257 and n1 != n2
    big, small = (m1, m2) if n1 > n2 else (m2, m1)
    # a smaller map behind a bigger snapshot: its normals, then zeros; a bigger map: cut at the snapshot's size
    snap = big.keyframe_snapshot()
    snap.add_normals(small)
    got, want = snap.normals(), unit_of(small.keylines())
    assert len(got) == big.size() and got[:len(want)].tobytes() == want.tobytes() and not got[len(want):].any()
    snap.add_normals(blank)
    assert not snap.normals().any()
    snap.release()
    snap = small.keyframe_snapshot()
    snap.add_normals(big)
    assert snap.normals().tobytes() == unit_of(big.keylines())[:small.size()].tobytes()
    snap.release()
    # gradient_norm not > 0 (zero, negative, NaN): (0, 0)
    kl = m1.keylines()
    kl["gradient_norm"][[3, 64, 255]] = (0.0, -2.0, np.nan)
    m1.upload(kl)
    snap = m1.keyframe_snapshot()
    snap.add_normals(m1)
    got = snap.normals()
    assert not got[[3, 64, 255]].any() and got.tobytes() == unit_of(kl).tobytes()
    snap.release()
    ctx.close()


def test_normals_refusals_and_resources(B):
    frames, cam = stream()
    live = B.test_live_resources()
    ctx, other = B.Context(params_for(B, cam, **KW_STREAM)), B.Context(params_for(B, cam, **KW_STREAM))
    maps = [ctx.detect_u8(frames[k], k * TS) for k in range(3)]
    foreign = other.detect_u8(frames[0], 0)
    L = B.lib()
    err = lambda: L.rebvio_hip_last_error().decode()
    n = C.c_int()
    snap = maps[0].keyframe_snapshot()
    base = B.test_live_resources()
    assert L.rebvio_hip_kf_snapshot_add_normals(snap.h, None) == -3 and "null" in err()
    assert L.rebvio_hip_kf_snapshot_add_normals(None, maps[0].h) == -3 and "null" in err()
    assert L.rebvio_hip_kf_snapshot_add_normals(snap.h, foreign.h) == -3 and "another context" in err()
    assert L.rebvio_hip_kf_snapshot_download_normals(snap.h, None, 0, C.byref(n)) == -7 and "no normals" in err()
    assert B.test_live_resources() == base                      # a refused call takes nothing
    snap.add_normals(maps[0])
    assert B.test_live_resources() == base + 1                  # one more buffer ...
    snap.add_normals(maps[0])
    assert B.test_live_resources() == base + 1                  # ... once
    assert L.rebvio_hip_kf_snapshot_download_normals(snap.h, None, 0, None) == -3 and "null" in err()
    assert L.rebvio_hip_kf_snapshot_download_normals(snap.h, None, -1, C.byref(n)) == -3 and "cap" in err()
    assert L.rebvio_hip_kf_snapshot_download_normals(snap.h, None, 4, C.byref(n)) == -3 and "cap" in err()
    buf = np.full((20, 2), -7.0, F32)
    assert L.rebvio_hip_kf_snapshot_download_normals(snap.h, buf.ctypes.data_as(C.POINTER(C.c_float)), 10, C.byref(n)) == 0
    assert n.value == maps[0].size() and buf[:10].tobytes() == unit_of(maps[0].keylines())[:10].tobytes() and (buf[10:] == -7.0).all()
    snap.release()
    assert B.test_live_resources() == base - 1                  # both buffers go with the snapshot
    # a map promised to R_prior_next has rotated gradients: -7, and nothing is taken
    c, s = F32(np.cos(0.01)), F32(np.sin(0.01))
    Rn = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], F32)
    snap = maps[1].keyframe_snapshot()
    mid = ctx.track_pair_begin(maps[0], maps[1])
    ctx.track_pair_finish_async(maps[0], maps[1], *vision_only_fusion(mid), R_prior_next=Rn)
    assert ctx.track_pair_result()[3] == 0
    held = B.test_live_resources()
    with pytest.raises(B.HipError) as e:
        snap.add_normals(maps[1])
    assert "error -7:" in str(e.value) and "R_prior_next" in str(e.value), str(e.value)
    assert B.test_live_resources() == held
    mid = ctx.track_pair_begin(maps[1], maps[2], R_prior=Rn)
    ctx.track_pair_finish_async(maps[1], maps[2], *vision_only_fusion(mid))
    assert ctx.track_pair_result()[3] == 0
    snap.add_normals(maps[2])
    gone = snap
    ctx.close()                                                 # the context frees both buffers of a snapshot that is still out
    assert L.rebvio_hip_kf_snapshot_add_normals(gone.h, maps[2].h) == -10 and "destroyed" in err()
    assert L.rebvio_hip_kf_snapshot_download_normals(gone.h, None, 0, C.byref(n)) == -10 and "destroyed" in err()
    gone.release()
    other.close()
    for m in maps + [foreign]:
        m.release()
    assert B.test_live_resources() == live


# ---- 2. sums and associations ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 800])
def test_sums_and_associations_on_crafted_snapshots(B, n):
    """the wave edge, the workgroup edge and several partials; at the crafted motion and at a random guess near it"""
    ctx, mk, mc, snap, D, A = crafted_scene(B, n)
    assert len(D[1]) == n
    R, t = true_motion()
    used = assert_evaluation(B, ctx, mc, snap, D, R, t, f"n {n}: truth")
    assert used >= 0.9 * len(A["prs4"]) and (n < 63 or len(A["prs4"]) >= 0.9 * n), (used, len(A["prs4"]))
    assert_evaluation(B, ctx, mc, snap, D, *random_guess(n), f"n {n}: random")
    assert_evaluation(B, ctx, mc, snap, D, *random_guess(n + 1), f"n {n}: other options", huber_px=0.7, min_cos=0.5, max_dist=6)
    snap.release()
    ctx.close()


def test_sums_without_normals_and_with_the_gate_off(B):
    ctx, mk, mc, snap, D, A = crafted_scene(B)
    bare = mk.keyframe_snapshot()                               # the same keyframe, no normals added
    Db = D[:3] + (None,) + D[4:]
    R, t = offset_guess(*OFFSETS[1])
    u_gate = assert_evaluation(B, ctx, mc, snap, D, R, t, "gate")
    u_off = assert_evaluation(B, ctx, mc, snap, D, R, t, "gate off", min_cos=-1.0)
    u_bare = assert_evaluation(B, ctx, mc, bare, Db, R, t, "no normals")
    print("used with the gate", u_gate, "gate off", u_off, "no normals", u_bare)
    assert u_gate < u_off == u_bare
    bare.release()
    snap.release()
    ctx.close()


def test_sums_over_256_partials(B):
    """keylines_max = 65 536 on a 2304 x 1900 frame (the frame of the pose tests' large case): a snapshot of 65 536 keylines, i.e. 256
    workgroup partials added up by k_kf_pose_step, against a detected map of that size"""
    Wb, Hb = 2304, 1900
    frames, cam = enlarged_stream(Wb, Hb, 3)
    ctx = B.Context(B.default_params(Hb, Wb, fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=60000, keylines_max=65536))
    maps = sorted((ctx.detect_u8(frames[i], i * 50000) for i in range(3)), key=lambda x: -x.size())
    mk, mc = maps[0], maps[1]
    print("keyframe", mk.size(), "current", mc.size())
    assert mk.size() == 65536 and mc.size() > 32768
    kl, cur = current_data(mc)
    A = craft_against(kl, cur[2], cur[3], 5, cam_of(ctx))
    base = mk.keylines()
    base["matches"] = 0
    n = min(len(A["prs4"]), len(base))
    assert n > 32768
    snap = snapshot_of(mk, craft_kf_keylines(base, A, n))
    D = data_of(ctx, snap, cur)
    R, t = true_motion()
    assert assert_evaluation(B, ctx, mc, snap, D, R, t, "large: truth") > 32768
    assert_evaluation(B, ctx, mc, snap, D, *random_guess(3), "large: random")
    snap.release()
    ctx.close()


# ---- 3. every skip rule, one keyline each ----------------------------------------------------------------------------------------
def test_every_skip_rule_drops_exactly_its_keyline(B):
    """Planted keyframe keylines with a control each, at R = I, t = (0, 0, -0.06): a keyline of rho 1 and pos_img = 0.94 (target -
    (cx, cy)) projects onto the target. The controls differ from their plant in the planted attribute only and are used."""
    frames, cam = stream()
    ctx = B.Context(params_for(B, cam, **KW_FULL))
    mk, mc = [ctx.detect_u8(frames[1 + k], k * TS) for k in range(2)]
    kl, cur = current_data(mc)
    pos, unit, ids, dists = cur[0], cur[1], cur[2].reshape(H, W), cur[3].reshape(H, W)
    tz = -0.06
    t = np.array([0.0, 0.0, tz])
    s = 1.0 + tz
    full = ids >= 0
    # cells: a rim cell inside the bounds whose neighbour outside is not empty either, per side; an empty cell; the farthest cell
    left = next(y for y in range(2, H - 2) if full[y, 0] and full[y, 1])
    right = next(y for y in range(2, H - 2) if full[y, W - 1] and full[y, W - 2])
    top = next(x for x in range(2, W - 2) if full[0, x] and full[1, x])
    bottom = next(x for x in range(2, W - 2) if full[H - 1, x] and full[H - 2, x])
    inner = np.zeros_like(full)
    inner[1:H - 1, 1:W - 1] = True
    ey, ex = np.argwhere(~full & inner)[0]
    far = np.where(full & inner, dists, -1)
    fy, fx = np.unravel_index(far.argmax(), far.shape)
    D_far = int(dists[fy, fx])
    controls_d = [dists[left, 1], dists[right, W - 2], dists[1, top], dists[H - 2, bottom]]
    assert D_far >= 2 and max(controls_d) < D_far, (D_far, controls_d)
    i0 = next(i for i in range(len(kl)) if inner[int(round(pos[i, 1])), int(round(pos[i, 0]))] and
              ids[int(round(pos[i, 1])), int(round(pos[i, 0]))] == i and np.abs(pos[i] - np.round(pos[i])).max() < 0.3)
    gy, gx = int(round(pos[i0, 1])), int(round(pos[i0, 0]))
    un = unit[i0].astype(np.float64)
    across = np.array([-un[1], un[0]])
    Z2 = (0.0, 0.0)
    #         name            target (x, y)        rho   matches normal  used
    plants = [("control",      (gx, gy),            1.0,  3,      un,     True),
              ("filter",       (gx, gy),            1.0,  1,      un,     False),
              ("Y.z",          (gx, gy),            19.0, 3,      un,     False),
              ("x = 0",        (0, left),           1.0,  3,      Z2,     False),
              ("x = 1",        (1, left),           1.0,  3,      Z2,     True),
              ("x = cols - 1", (W - 1, right),      1.0,  3,      Z2,     False),
              ("x = cols - 2", (W - 2, right),      1.0,  3,      Z2,     True),
              ("y = 0",        (top, 0),            1.0,  3,      Z2,     False),
              ("y = 1",        (top, 1),            1.0,  3,      Z2,     True),
              ("y = rows - 1", (bottom, H - 1),     1.0,  3,      Z2,     False),
              ("y = rows - 2", (bottom, H - 2),     1.0,  3,      Z2,     True),
              ("empty cell",   (ex, ey),            1.0,  3,      Z2,     False),
              ("max_dist",     (fx, fy),            1.0,  3,      Z2,     None),
              ("gate: across", (gx, gy),            1.0,  3,      across, False),
              ("gate: against", (gx, gy),           1.0,  3,      -un,    False),
              ("zero normal",  (gx, gy),            1.0,  3,      Z2,     True)]
    base = mk.keylines()
    assert len(base) >= len(plants)
    base["matches"] = 0                                          # every other keyframe keyline is filtered out
    kf = base.copy()
    for k, (name, (x, y), rho, mt, nrm, _) in enumerate(plants):
        # Y.z plant: rho 19 gives Y.z = 1 - 1.14 < 0 wherever it points
        kf["pos_img"][k] = (F32(s * (x + 0.2 - ctx.p.cx)), F32(s * (y - 0.2 - ctx.p.cy)))
        kf["rho"][k], kf["sigma_rho"][k], kf["matches"][k] = rho, 0.05 * rho, mt
        kf["gradient"][k] = (F32(10 * nrm[0]), F32(10 * nrm[1]))
        kf["gradient_norm"][k] = 10.0 if (nrm[0] or nrm[1]) else 0.0
    snap = snapshot_of(mk, kf)
    D = data_of(ctx, snap, cur)
    assert not D[3][[k for k, p in enumerate(plants) if p[4] is Z2]].any()
    for max_dist, far_used in ((D_far - 1, False), (D_far, True)):
        _, _, used, assoc, g = np_kf_align_sums(*D, np.eye(3), t, max_dist=max_dist)
        assert min(g.values()) > GUARD, g
        got, a = mc.keyframe_align(snap, B.default_kf_align_opts(ctx, max_iter=0, max_dist=max_dist), np.eye(3), t, want_assoc=True)
        assert np.array_equal(a, assoc)
        want = [far_used if u is None else u for *_, u in plants]
        assert [(x >= 0) for x in a[:len(plants)]] == want, [(p[0], x) for p, x in zip(plants, a)]
        assert (a[len(plants):] == -1).all() and got.used == sum(want) == used
        for k, (name, (x, y), *_rest) in enumerate(plants):
            assert a[k] in (-1, ids[y, x]), (name, a[k], ids[y, x])
    snap.release()
    ctx.close()


# ---- 4. the solve --------------------------------------------------------------------------------------------------------------------
def test_solve_from_the_offsets(B):
    ctx, mk, mc, snap, D, A = crafted_scene(B)
    worst = 0.0
    for rot, tr in ((0.0, 0.0),) + OFFSETS:
        R0, t0 = offset_guess(rot, tr)
        ref = np_kf_align(*D, R0, t0)
        assert ref["guard"] > GUARD, ref["guard"]
        got, assoc = mc.keyframe_align(snap, None, R0, t0, want_assoc=True)
        e_np, e_dev, d = pose_err(ref["R"], ref["t"]), pose_err(got.R, got.t), pose_err(got.R, got.t, ref["R"], ref["t"])
        worst = max(worst, d)
        print(f"offset ({rot}, {tr}): err np {e_np:.3g} device {e_dev:.3g} |device - np| {d:.3g} used {got.used} of {got.candidates} "
              f"cond(H) {np.linalg.cond(ref['H']):.1f} guard {ref['guard']:.3g}")
        assert ref["status"] == 0 == got.status and got.iterations == 8 == ref["iterations"]
        assert got.used == ref["used"] and got.candidates == len(D[1]) and np.array_equal(assoc, ref["assoc"])
        assert e_np <= 1e-5                                      # the restatement converges from here, with the gradient test
        assert DEV_VS_NP <= 0.1 * e_np
        assert d <= DEV_VS_NP
        # H, g, cost, used and assoc are those of the returned pose
        S, absS, used, a2, _ = np_kf_align_sums(*D, np.array(got.R), np.array(got.t))
        assert used == got.used and np.array_equal(a2, assoc)
        assert (np.abs(pose_sums(got) - S) <= (used + 64) * 2.0 ** -52 * absS).all()
        assert same_bytes(got, mc.keyframe_align(snap, None, R0, t0))
    print(f"max |device - np| {worst:.3g}")
    snap.release()
    ctx.close()


def test_solve_with_displaced_keylines_follows_the_restatement(B):
    """20 % of the keyframe keylines displaced by 15 px along their normal: device == restatement, no bound on the recovered error"""
    ctx, mk, mc, snap, D, A = crafted_scene(B, displaced=0.2)
    for rot, tr in OFFSETS:
        R0, t0 = offset_guess(rot, tr)
        ref = np_kf_align(*D, R0, t0)
        assert ref["guard"] > GUARD, ref["guard"]
        got, assoc = mc.keyframe_align(snap, None, R0, t0, want_assoc=True)
        print(f"displaced, offset ({rot}, {tr}): err np {pose_err(ref['R'], ref['t']):.3g} device {pose_err(got.R, got.t):.3g} "
              f"|device - np| {pose_err(got.R, got.t, ref['R'], ref['t']):.3g} used {got.used} of {got.candidates}")
        assert got.status == ref["status"] == 0 and got.iterations == ref["iterations"] and got.used == ref["used"]
        assert np.array_equal(assoc, ref["assoc"])
        assert pose_err(got.R, got.t, ref["R"], ref["t"]) <= DEV_VS_NP
    snap.release()
    ctx.close()


# ---- 5. statuses, launches, refusals, resources -------------------------------------------------------------------------------------
def test_statuses(B):
    R0, t0 = offset_guess(*OFFSETS[0])
    # used < min_used at the first evaluation: status 3, pose = guess, the sums of the guess still returned
    ctx, mk, mc, snap, D, A = crafted_scene(B, 11)
    got, assoc = mc.keyframe_align(snap, None, R0, t0, want_assoc=True)
    S, absS, used, a2, _ = np_kf_align_sums(*D, R0, t0)
    assert (got.status, got.iterations, got.candidates) == (3, 0, 11) and got.used == used <= 11 and np.array_equal(assoc, a2)
    assert np.array_equal(np.array(got.R), R0.reshape(9)) and np.array_equal(np.array(got.t), t0)
    assert (np.abs(pose_sums(got) - S) <= (used + 64) * 2.0 ** -52 * absS).all()
    R, t = true_motion()
    ok = mc.keyframe_align(snap, B.default_kf_align_opts(ctx, min_used=1), R, t)
    assert ok.used >= 1 and ok.status in (0, 2)                   # (min_used passed; up to 11 terms may or may not factor)
    snap.release()
    ctx.close()
    # no term at all with min_used 0: H = 0 does not factor - status 2, pose = guess, nothing non-finite
    ctx, mk, mc, snap, D, A = crafted_scene(B, 64)
    o = B.default_kf_align_opts(ctx, min_used=0, kf_filter=dict(min_matches=100))
    got, assoc = mc.keyframe_align(snap, o, R0, t0, want_assoc=True)
    assert np_kf_align(*D, R0, t0, flt=(100, 0.5, 1e-3, 20.0), min_used=0)["status"] == 2
    assert (got.status, got.iterations, got.used, got.candidates) == (2, 0, 0, 64) and (assoc == -1).all()
    assert np.array_equal(np.array(got.R), R0.reshape(9)) and np.array_equal(np.array(got.t), t0)
    assert np.isfinite(np.frombuffer(bytes(got), np.float64, 55)).all() and not np.array(got.H).any()
    snap.release()
    ctx.close()


def test_an_empty_snapshot_launches_nothing(B):
    ctx, (mk, mc) = sized_maps(B, 0)
    snap = mk.keyframe_snapshot()
    snap.add_normals(mk)
    assert snap.download()[0].shape == (0, 4) and snap.normals().shape == (0, 2)
    base = B.test_live_resources()
    ctx.profile_reset()
    ctx.profile(True)
    R0, t0 = offset_guess(*OFFSETS[0])
    got, assoc = mc.keyframe_align(snap, None, R0, t0, want_assoc=True)
    launches = {name: calls for name, (_, calls) in ctx.profile_read().items() if calls}
    ctx.profile(False)
    assert launches == {} and B.test_live_resources() == base, launches
    assert (got.status, got.candidates, got.used, got.iterations) == (3, 0, 0, 0) and len(assoc) == 0
    assert np.array_equal(np.array(got.R), R0.reshape(9)) and np.array_equal(np.array(got.t), t0)
    assert not np.array(got.H).any() and not np.array(got.g).any() and got.cost == 0.0
    snap.release()
    ctx.close()


def test_the_entries_launch_what_they_document(B):
    """max_iter + 1 evaluations of two kernels each and none of the correspondence kernels; one kernel for the normals"""
    ctx, mk, mc, snap, D, A = crafted_scene(B, 65)
    ctx.profile_reset()
    ctx.profile(True)
    mc.keyframe_align(snap, B.default_kf_align_opts(ctx, max_iter=5))
    launches = {name: calls for name, (_, calls) in ctx.profile_read().items() if calls}
    assert launches == dict(k_kf_align_sums=6, k_kf_pose_step=6), launches
    ctx.profile_reset()
    mc.keyframe_align(snap, B.default_kf_align_opts(ctx, max_iter=0))
    snap.add_normals(mk)
    launches = {name: calls for name, (_, calls) in ctx.profile_read().items() if calls}
    ctx.profile(False)
    assert launches == dict(k_kf_align_sums=1, k_kf_pose_step=1, k_kf_snapshot_normals=1), launches
    snap.release()
    ctx.close()


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
    out = B.KfPose()
    base = B.test_live_resources()
    assert L.rebvio_hip_map_keyframe_align(None, snap.h, None, None, None, C.byref(out), None) == -3 and "null" in err()
    assert L.rebvio_hip_map_keyframe_align(maps[1].h, None, None, None, None, C.byref(out), None) == -3 and "null" in err()
    assert L.rebvio_hip_map_keyframe_align(maps[1].h, snap.h, None, None, None, None, None) == -3 and "null" in err()
    assert L.rebvio_hip_map_keyframe_align(maps[1].h, fsnap.h, None, None, None, C.byref(out), None) == -3 and "another context" in err()
    nan_R = np.eye(3)
    nan_R[2, 0] = np.nan
    d = lambda **kw: dict(opts=B.default_kf_align_opts(ctx, **kw))
    sr = int(ctx.p.search_range)
    for kw, word in ((dict(R0=nan_R), "non-finite"), (dict(t0=[0.0, 0.0, -np.inf]), "non-finite"), (d(huber_px=0.0), "huber_px"),
                     (d(huber_px=float("nan")), "huber_px"), (d(max_iter=33), "max_iter"), (d(max_iter=-1), "max_iter"), (d(min_used=-1), "min_used"),
                     (d(min_used=65537), "min_used"), (d(min_cos=1.5), "min_cos"), (d(min_cos=-1.5), "min_cos"), (d(min_cos=float("nan")), "min_cos"),
                     (d(max_dist=-1), "max_dist"), (d(max_dist=sr + 1), "max_dist"), (d(kf_filter=dict(rho_min=-1.0)), "rho_min"),
                     (d(kf_filter=dict(max_rel_sigma=float("nan"))), "NaN")):
        with pytest.raises(B.HipError) as e:
            maps[1].keyframe_align(snap, **kw)
        assert "error -3:" in str(e.value) and word in str(e.value), (kw, str(e.value))
    assert B.test_live_resources() == base                      # nothing was allocated by a refused call
    assert B.default_kf_align_opts(ctx).max_dist == sr
    got = maps[1].keyframe_align(snap, B.default_kf_align_opts(ctx, max_dist=sr, min_cos=1.0, max_iter=32, min_used=65536))
    assert got.status == 3                                      # the bounds themselves are legal
    assert B.test_live_resources() == base + 1                  # the scratch: ONE allocation on first use ...
    maps[1].keyframe_align(snap)
    maps[2].keyframe_align(snap, want_assoc=True)
    assert B.test_live_resources() == base + 1                  # ... and kept
    # a map promised to R_prior_next is accepted: pos, unit and the field are not rotated
    kl1, cur1 = current_data(maps[1])
    c, s = F32(np.cos(0.01)), F32(np.sin(0.01))
    Rn = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], F32)
    mid = ctx.track_pair_begin(maps[0], maps[1])
    ctx.track_pair_finish_async(maps[0], maps[1], *vision_only_fusion(mid), R_prior_next=Rn)
    assert ctx.track_pair_result()[3] == 0
    with pytest.raises(B.HipError, match="error -7:"):
        maps[1].keyframe_pose(snap)                             # (the chain pose refuses it)
    D = data_of(ctx, snap, cur1)
    o = B.default_kf_align_opts(ctx, max_iter=0, kf_filter=dict(min_matches=0, max_rel_sigma=1e9, rho_min=1e-6, rho_max=1e6))
    got, assoc = maps[1].keyframe_align(snap, o, want_assoc=True)
    S, absS, used, a2, g = np_kf_align_sums(*D, np.eye(3), np.zeros(3), flt=(0, 1e9, 1e-6, 1e6))
    assert min(g.values()) > GUARD and used > 100
    assert got.used == used and np.array_equal(assoc, a2) and (np.abs(pose_sums(got) - S) <= (used + 64) * 2.0 ** -52 * absS).all()
    mid = ctx.track_pair_begin(maps[1], maps[2], R_prior=Rn)
    ctx.track_pair_finish_async(maps[1], maps[2], *vision_only_fusion(mid))
    assert ctx.track_pair_result()[3] == 0
    after = maps[1].keylines()
    assert np.array_equal(after["pos"], kl1["pos"]) and (after["gradient"] != kl1["gradient"]).any()     # what is read is not what tracking writes
    # an uploaded current map: its unit is detection's, its field is not - refused
    maps[2].upload(maps[2].keylines())
    with pytest.raises(B.HipError, match="error -7:.*distance field"):
        maps[2].keyframe_align(snap)
    ctx.close()
    assert L.rebvio_hip_map_keyframe_align(maps[1].h, snap.h, None, None, None, C.byref(out), None) == -10 and "destroyed" in err()
    assert L.rebvio_hip_map_keyframe_align(foreign.h, snap.h, None, None, None, C.byref(out), None) == -10 and "destroyed" in err()
    snap.release()
    fsnap.release()
    other.close()
    for m in maps + [foreign]:
        m.release()
    assert B.test_live_resources() == live


# ---- 6. the real stream --------------------------------------------------------------------------------------------------------------
def test_a_keyframe_is_found_again_after_a_reset(B):
    """Mark and snapshot frame 2 with normals, track four pairs: the chain pose P is status 0. After rebvio_hip_reset_state and a new
    detection of the same frame the chain is gone (0 candidates, status 3); the alignment warm-started from P has a pose to give.
    Only device == restatement is asserted of that pose (DESIGN.md 5i reports where it lands)."""
    frames, cam = stream()
    ctx = B.Context(params_for(B, cam, **KW_STREAM))
    maps = [ctx.detect_u8(frames[k], k * TS) for k in range(7)]
    for k in range(6):
        assert ctx.track_pair(maps[k], maps[k + 1]).status == 0
        if k == 1:
            maps[2].mark_keyframe()
            snap = maps[2].keyframe_snapshot()
            snap.add_normals(maps[2])
    P = maps[6].keyframe_pose(snap)
    assert P.status == 0 and P.used >= 12
    ctx.reset_state()
    again = ctx.detect_u8(frames[6], 7 * TS)
    lost = again.keyframe_pose(snap)
    assert (lost.candidates, lost.status) == (0, 3)
    kl, cur = current_data(again)
    D = data_of(ctx, snap, cur)
    for what, R0, t0 in (("from P", np.array(P.R).reshape(3, 3), np.array(P.t)), ("from the identity", np.eye(3), np.zeros(3))):
        ref = np_kf_align(*D, R0, t0)
        assert ref["guard"] > GUARD, (what, ref["guard"])
        got, assoc = again.keyframe_align(snap, None, R0, t0, want_assoc=True)
        d = pose_err(got.R, got.t, ref["R"], ref["t"])
        print(f"{what}: status {got.status} used {got.used} of {got.candidates} cost {got.cost:.1f} |pose - P| {pose_err(got.R, got.t, P.R, P.t):.3g} "
              f"|device - np| {d:.3g} (chain: used {P.used} of {P.candidates})")
        assert got.status == ref["status"] and got.used == ref["used"] and got.iterations == ref["iterations"]
        assert np.array_equal(assoc, ref["assoc"]) and d <= DEV_VS_NP
        if what == "from P":
            assert got.status == 0 and got.used >= 12
    snap.release()
    ctx.close()


def test_alignment_calls_between_pairs_disturb_nothing(B):
    """the pair records and the final keylines of the stream are equal word for word with and without normals and alignment calls
    between the pairs"""
    frames, cam = stream()

    def run(with_align):
        ctx = B.Context(params_for(B, cam, **KW_STREAM))
        maps = [ctx.detect_u8(frames[k], k * TS) for k in range(9)]
        recs, snap, R, t = [], None, None, None
        for k in range(8):
            out = ctx.track_pair(maps[k], maps[k + 1])
            recs.append(rec(out, maps[k + 1].size()))
            if k == 1:
                maps[2].mark_keyframe()          # (marked in both runs: the ids are part of what is compared)
                if with_align:
                    snap = maps[2].keyframe_snapshot()
                    snap.add_normals(maps[2])
            if k >= 2 and with_align:
                got = maps[k + 1].keyframe_align(snap, None, R, t)
                maps[k].keyframe_align(snap, None, R, t)          # an older map too
                print(f"pair {k}: used {got.used} of {got.candidates} status {got.status} |t| {np.linalg.norm(got.t):.4f} cost {got.cost:.1f}")
                if got.status == 0:
                    R, t = np.array(got.R), np.array(got.t)
        final = maps[8].keylines()
        if snap:
            snap.release()
        ctx.close()
        return recs, final

    plain, kl_plain = run(False)
    aligned, kl_aligned = run(True)
    same_records(plain, aligned, "with and without normals and alignment calls")
    assert_keylines_equal(kl_plain, kl_aligned, "final keylines")


# ---- the refusal table: every shared refusal with its code and whole text; which one wins when several apply ------

ALIGN, NORMALS = "map_keyframe_align", "kf_snapshot_add_normals"
_ao = lambda s, **kw: s.B.default_kf_align_opts(s.ctx, **kw)
REFUSED = {
    "destroyed map": (lambda s: s.dm.keyframe_align(s.dsnap), -10, DEAD_MAP),
    "destroyed snapshot": (lambda s: s.m.keyframe_align(s.dsnap), -10, DEAD_SNAPSHOT),
    "foreign snapshot": (lambda s: s.m.keyframe_align(s.fsnap), -3, foreign_snapshot(ALIGN)),
    "no field": (lambda s: s.up.keyframe_align(s.snap), -7, no_field(ALIGN)),
    "R0 not finite": (lambda s: s.m.keyframe_align(s.snap, None, s.nan_R), -3, f"{ALIGN}: non-finite R0 or t0"),
    "t0 not finite": (lambda s: s.m.keyframe_align(s.snap, None, None, s.inf_t), -3, f"{ALIGN}: non-finite R0 or t0"),
    "min_cos above": (lambda s: s.m.keyframe_align(s.snap, _ao(s, min_cos=1.5)), -3, f"{ALIGN}: min_cos outside [-1, 1]"),
    "min_cos NaN": (lambda s: s.m.keyframe_align(s.snap, _ao(s, min_cos=float("nan"))), -3, f"{ALIGN}: min_cos outside [-1, 1]"),
    "max_dist below": (lambda s: s.m.keyframe_align(s.snap, _ao(s, max_dist=-1)), -3, f"{ALIGN}: max_dist outside 0..search_range"),
    "max_dist above": (lambda s: s.m.keyframe_align(s.snap, _ao(s, max_dist=s.sr + 1)), -3, f"{ALIGN}: max_dist outside 0..search_range"),
    "wins: a foreign snapshot over an option and no field": (lambda s: s.up.keyframe_align(s.fsnap, _ao(s, min_cos=2.0), s.nan_R), -3,
                                                             foreign_snapshot(ALIGN)),
    "wins: a destroyed snapshot over an option": (lambda s: s.m.keyframe_align(s.dsnap, _ao(s, max_dist=-1)), -10, DEAD_SNAPSHOT),
    "wins: a destroyed map over a foreign snapshot": (lambda s: s.dm.keyframe_align(s.snap), -10, DEAD_MAP),
    "wins: a guess over min_cos": (lambda s: s.m.keyframe_align(s.snap, _ao(s, min_cos=2.0), s.nan_R), -3, f"{ALIGN}: non-finite R0 or t0"),
    "wins: min_cos over max_dist": (lambda s: s.m.keyframe_align(s.snap, _ao(s, min_cos=2.0, max_dist=-1)), -3,
                                    f"{ALIGN}: min_cos outside [-1, 1]"),
    "wins: an option over no field": (lambda s: s.up.keyframe_align(s.snap, _ao(s, max_dist=-1)), -3, f"{ALIGN}: max_dist outside 0..search_range"),
    "normals: destroyed map": (lambda s: s.dsnap.add_normals(s.dm), -10, DEAD_MAP),
    "normals: destroyed snapshot": (lambda s: s.dsnap.add_normals(s.m), -10, DEAD_SNAPSHOT),
    "normals: foreign snapshot": (lambda s: s.fsnap.add_normals(s.m), -3, f"{NORMALS}: map of another context"),
    "normals: wins: a destroyed map over a foreign snapshot": (lambda s: s.snap.add_normals(s.dm), -10, DEAD_MAP),
    "normals: download from a destroyed snapshot": (lambda s: s.dsnap.normals(), -10, DEAD_SNAPSHOT),
}

@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusal_table(refusal_scene, case):
    """every refusal of the table with its return code and its whole rebvio_hip_last_error text; nothing is allocated"""
    assert_refused(refusal_scene, *REFUSED[case])
