"""Depth fusion into a keyframe snapshot on the device: rebvio_hip_kf_snapshot_fuse_depth (k_kf_fuse_depth). The contracts:
  - every output word - the snapshot's records and matches, assoc, the six counts - equals the host hook's
    (rebvio_hip_test_kf_fuse_host) and the numpy restatement's (tests/kf_fuse_ref.py) on the snapshot, keylines and distance field
    downloaded just before: per-keyline IEEE fp64 in the same order on all sides and no sum whose order could differ, so equality is
    the bound. Wave and workgroup edges, and 65 536 keylines for the grid at its cap;
  - two snapshots fused alike are equal in every byte, and a second fusion works on what the first left;
  - every outcome of the definition planted on a detected map is what comes out for exactly that keyline;
  - t = 0 and an empty snapshot change nothing; launches, resources and refusals are as include/rebvio_hip.h documents;
  - the alignment afterwards sees the fused depths, and nothing of tracking is disturbed.
A comparison is valid only while no keyline of the restatement comes within GUARD of a decision; every comparison asserts that
first. The keyframe keylines are crafted against the current map (craft_against), their rho perturbed within sigma_rho, uploaded into
another map of the same context and snapshotted. All maps are 160x120 with keylines_max <= 800 unless a case says otherwise."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import params_for
from kf_align_ref import GUARD, OFFSETS, craft_against, craft_kf_keylines, np_kf_align, offset_guess, unit_of
from kf_fuse_ref import INT_MIN, counts_of, np_kf_fuse, perturbed
from kf_pose_ref import pose_err, true_motion
from support import B, refusal_scene  # noqa: F401
from support import DEAD_MAP, DEAD_SNAPSHOT, assert_refused, foreign_snapshot, no_field
from support import F32, TS, enlarged_stream, rec, same_records

pytestmark = pytest.mark.gpu

W, H, NF = 160, 120, 10
KW_STREAM = dict(keylines_ref=600, keylines_max=800, global_min_matches_threshold=50)      # the stream of the pose tests: every pair tracks
DEV_VS_NP = 2.22e-14        # |device - numpy| over R and t of an alignment's solve: the bound of tests/test_keyframe_align_gpu.py
WIDE = (0, 1e9, 1e-3, 20.0)


@functools.lru_cache(maxsize=None)
def stream():
    from rebvio_amd import synth
    return synth.render_stream(W, H, NF)


def cam_of(ctx):
    return (ctx.p.fm, ctx.p.cx, ctx.p.cy, ctx.rows, ctx.cols)


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


def current_data(mc):
    """what the restatement is given of the current map: pos, unit, the field - downloaded"""
    kl = mc.keylines()
    ids, dists = mc.distance_field()
    return kl, (np.ascontiguousarray(kl["pos"]), unit_of(kl), ids.reshape(-1), dists.reshape(-1))


def snapshot_of(mk, kf_keylines, normals=True):
    mk.upload(kf_keylines)
    snap = mk.keyframe_snapshot()
    if normals:
        snap.add_normals(mk)
    return snap


def crafted(B, ctx, mk, mc, seed=1):
    """(restatement data of the current map, keyline array of the keyframe): crafted against mc, rho perturbed within sigma_rho;
    keyframe keylines behind the crafted ones are filtered out (matches 0)"""
    kl, cur = current_data(mc)
    A = dict(craft_against(kl, cur[2], cur[3], seed, cam_of(ctx)))
    A["prs4"], _ = perturbed(A, seed + 100)
    base = mk.keylines()
    base["matches"] = 0
    return cur, craft_kf_keylines(base, A, min(len(A["prs4"]), len(base)))


def data_of(ctx, snap, cur, normals=True):
    prs4, mt = snap.download()
    return (cam_of(ctx), prs4, mt, snap.normals() if normals else None, *cur)


def np_opts(kw):
    o = dict(kw)
    if "kf_filter" in o:
        f = o.pop("kf_filter")
        o["flt"] = tuple(f[k] for k in ("min_matches", "max_rel_sigma", "rho_min", "rho_max"))
    return o


def wide():
    return dict(zip(("min_matches", "max_rel_sigma", "rho_min", "rho_max"), WIDE))


def assert_fusion(B, ctx, mc, snap, D, R, t, what, **kw):
    """one fusion on the device against the restatement and the hook run on D, the snapshot's download from just before: the guards,
    then every output word. Returns the restatement."""
    ref = np_kf_fuse(*D, R, t, **np_opts(kw))
    assert min(ref["guards"].values()) > GUARD, (what, ref["guards"])
    hk, hp, hm, ha = B.kf_fuse_host(*D[0], int(ctx.p.search_range), *D[1:], B.default_kf_fuse_opts(ctx, **kw), R, t)
    got, assoc = snap.fuse_depth(mc, R, t, B.default_kf_fuse_opts(ctx, **kw), want_assoc=True)
    prs4, mt = snap.download()
    for side, (cn, p, m, a) in (("hook", (hk, hp, hm, ha)), ("device", (got, prs4, mt, assoc))):
        assert counts_of(cn) == counts_of(ref), (what, side, counts_of(cn), counts_of(ref))
        assert np.array_equal(a, ref["assoc"]), (what, side, np.flatnonzero(a != ref["assoc"])[:8])
        assert p.tobytes() == ref["prs4"].tobytes(), (what, side, np.flatnonzero((p != ref["prs4"]).any(1))[:8])
        assert np.array_equal(m, ref["matches"]), (what, side)
    assert got.associated == got.fused + got.gated + got.flat and got.candidates == len(D[1])
    return ref


# ---- 1. device == hook == restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 800])
def test_fusion_on_crafted_snapshots_bit_for_bit(B, n):
    """the wave edge, the workgroup edge and several workgroups; a second fusion with other options follows the restatement applied
    twice: the state is carried across calls"""
    ctx, (mk, mc) = sized_maps(B, n)
    cur, kf = crafted(B, ctx, mk, mc)
    snap = snapshot_of(mk, kf)
    R, t = true_motion()
    D = data_of(ctx, snap, cur)
    assert len(D[1]) == n
    first = assert_fusion(B, ctx, mc, snap, D, R, t, f"n {n}: first")
    assert n < 63 or first["fused"] >= 0.7 * n, counts_of(first)
    D2 = data_of(ctx, snap, cur)
    assert D2[1].tobytes() == first["prs4"].tobytes()
    second = assert_fusion(B, ctx, mc, snap, D2, R, t, f"n {n}: second", gate_sigma=0.8, q_abs=0.02, pixel_sigma=0.5, max_dist=6)
    assert (second["matches"][second["assoc"] >= 0] >= 4).all() and (n < 63 or (second["matches"] == 5).sum() >= 0.7 * n)
    assert snap.normals().tobytes() == D[3].tobytes()                          # the normals are never written
    assert np.array_equal(snap.download()[0][:, :2], D[1][:, :2])              # nor pos_img
    snap.release()
    ctx.close()


def test_fusion_over_the_capped_grid(B):
    """keylines_max = 65 536 on a 2304 x 1900 frame (the frame of the alignment's large case): the grid at its cap of 256 workgroups,
    the largest snapshot a context can hold"""
    Wb, Hb = 2304, 1900
    frames, cam = enlarged_stream(Wb, Hb, 3)
    ctx = B.Context(B.default_params(Hb, Wb, fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=60000, keylines_max=65536))
    maps = sorted((ctx.detect_u8(frames[i], i * 50000) for i in range(3)), key=lambda x: -x.size())
    mk, mc = maps[0], maps[1]
    assert mk.size() == 65536 and mc.size() > 32768
    cur, kf = crafted(B, ctx, mk, mc, seed=5)
    snap = snapshot_of(mk, kf)
    R, t = true_motion()
    ref = assert_fusion(B, ctx, mc, snap, data_of(ctx, snap, cur), R, t, "large")
    print("large:", counts_of(ref))
    n_crafted = int((kf["matches"] > 0).sum())
    assert n_crafted > 32768 and ref["candidates"] == 65536
    # keylines of the first and of the last workgroups are fused (at 4 x the focal length the perturbed depths move many off their owners)
    assert (ref["assoc"][:32768] >= 0).sum() > 1000 and (ref["assoc"][32768:] >= 0).sum() > 1000
    snap.release()
    ctx.close()


def test_two_snapshots_fused_alike_are_byte_identical(B):
    ctx, (mk, mc) = sized_maps(B, 800)
    cur, kf = crafted(B, ctx, mk, mc)
    a, b = snapshot_of(mk, kf), snapshot_of(mk, kf)
    R, t = true_motion()
    outs = []
    for s in (a, b, a, b):
        got, assoc = s.fuse_depth(mc, R, t, want_assoc=True)
        outs.append((bytes(got), assoc.tobytes(), *(x.tobytes() for x in s.download())))
    assert outs[0] == outs[1] and outs[2] == outs[3] and outs[0] != outs[2]
    a.release()
    b.release()
    ctx.close()


@pytest.mark.parametrize("case", ["no normals", "min_cos -1"])
def test_fusion_without_the_gradient_test(B, case):
    ctx, (mk, mc) = sized_maps(B, 800)
    cur, kf = crafted(B, ctx, mk, mc)
    R, t = offset_guess(*OFFSETS[1])                          # off the truth: crossing edges take some keylines
    gated = snapshot_of(mk, kf)
    with_gate = assert_fusion(B, ctx, mc, gated, data_of(ctx, gated, cur), R, t, "gate")
    if case == "no normals":
        snap = snapshot_of(mk, kf, normals=False)
        with pytest.raises(B.HipError, match="error -7:"):
            snap.normals()
        ref = assert_fusion(B, ctx, mc, snap, data_of(ctx, snap, cur, normals=False), R, t, case)
    else:
        snap = snapshot_of(mk, kf)
        ref = assert_fusion(B, ctx, mc, snap, data_of(ctx, snap, cur), R, t, case, min_cos=-1.0)
    print(case, counts_of(ref), "with the gate", counts_of(with_gate))
    assert ref["associated"] > with_gate["associated"]
    gated.release()
    snap.release()
    ctx.close()


# ---- 2. every outcome, one keyline each ---------------------------------------------------------------------------------------------
def test_every_outcome_planted_on_a_detected_map(B):
    """Planted keyframe keylines at R = I, t = (0.02, 0.01, 0): Y.z = 1, a keyline of depth rho and pos_img = target - (cx, cy) -
    fm rho t projects onto the target pixel, and against an owner of unit n there  e = n . (offset from the owner's pos),
    h = fm n . t. The owner i0 sits within 0.15 px of its cell's centre and every plant 0.3 px off it along n, so all land in
    i0's cell with |e| = 0.3. The gate is |e| / 1.2: sigma_rho 0.4 (S = 1 + 0.16 h^2 >= 1.64 for |h| >= 2) passes it, 1e-3 (S = 1)
    does not. rho_n = rho - K e: a plant on the side where h e > 0 moves down, on the other side up."""
    frames, cam = stream()
    ctx = B.Context(params_for(B, cam, keylines_ref=600, keylines_max=800, global_min_matches_threshold=1))
    mk, mc = [ctx.detect_u8(frames[1 + k], k * TS) for k in range(2)]
    kl, cur = current_data(mc)
    pos, unit, ids, dists = cur[0], cur[1], cur[2].reshape(H, W), cur[3].reshape(H, W)
    fm, cx, cy = ctx.p.fm, ctx.p.cx, ctx.p.cy
    t = np.array([0.02, 0.01, 0.0])

    def good(i):
        x, y = int(round(pos[i, 0])), int(round(pos[i, 1]))
        return (2 <= x <= W - 3 and 2 <= y <= H - 3 and ids[y, x] == i and np.abs(pos[i] - np.round(pos[i])).max() < 0.15 and
                abs(fm * (unit[i].astype(np.float64) @ t[:2])) >= 2.0)
    i0 = next(i for i in range(len(kl)) if good(i))
    un = unit[i0].astype(np.float64)
    sh = np.sign(un @ t[:2])
    #         name              side  rho     sigma   matches  outcome   clamped
    plants = [("fused",          +1,  1.0,    0.4,    3,       "fused",  False),
              ("fused, other",   -1,  1.0,    0.4,    3,       "fused",  False),
              ("gated",          +1,  1.0,    1e-3,   3,       "gated",  False),
              ("flat",           +1,  1.0,    0.0,    3,       "flat",   False),
              ("clamped low",    sh,  0.002,  1.0,    3,       "fused",  True),
              ("low, other",     -sh, 0.002,  1.0,    3,       "fused",  False),
              ("clamped high",   -sh, 19.99,  5.0,    3,       "fused",  True),
              ("high, other",    sh,  19.99,  5.0,    3,       "fused",  False),
              ("rho_max",        +1,  25.0,   0.4,    3,       "none",   False),
              ("NaN sigma_rho",  +1,  1.0,    np.nan, 3,       "none",   False),
              ("saturated",      +1,  1.0,    0.4,    0xFFFFFFFF, "fused", False)]
    base = mk.keylines()
    base["matches"] = 0                                          # with min_matches 1 every other keyframe keyline is filtered out
    kf = base.copy()
    for k, (name, side, rho, sig, mt, *_) in enumerate(plants):
        target = pos[i0].astype(np.float64) + 0.3 * side * un
        kf["pos_img"][k] = (F32(target[0] - cx - fm * rho * t[0]), F32(target[1] - cy - fm * rho * t[1]))
        kf["rho"][k], kf["sigma_rho"][k], kf["matches"][k] = rho, sig, mt
        kf["gradient"][k] = (F32(10 * un[0]), F32(10 * un[1]))
        kf["gradient_norm"][k] = 10.0
    snap = snapshot_of(mk, kf)
    D = data_of(ctx, snap, cur)
    flt = dict(wide(), min_matches=1)
    ref = assert_fusion(B, ctx, mc, snap, D, np.eye(3), t, "plants", kf_filter=flt, gate_sigma=0.3 / 1.2)
    P = len(plants)
    assert np.allclose(np.abs(ref["e"][[0, 1, 2, 3]]), 0.3, atol=1e-3) and abs(ref["h"][0]) >= 2.0
    want = {"fused": i0, "gated": -1 - i0, "flat": -1 - i0, "none": INT_MIN}
    assert ref["assoc"][:P].tolist() == [want[p[5]] for p in plants], list(zip([p[0] for p in plants], ref["assoc"][:P]))
    assert (ref["assoc"][P:] == INT_MIN).all()
    fused = sum(p[5] == "fused" for p in plants)
    assert counts_of(ref) == (len(kf), P - 2, fused, 1, 1, 2)
    after, before = ref["prs4"], D[1]
    for k, (name, side, rho, sig, mt, outcome, clamped) in enumerate(plants):
        if outcome != "fused":
            assert after[k].tobytes() == before[k].tobytes() and ref["matches"][k] == D[2][k], name
            continue
        assert ref["matches"][k] == min(mt + 1, 0xFFFFFFFF), name
        assert (after[k, 2] in (F32(1e-3), F32(20.0))) == clamped, (name, after[k])
        assert clamped or F32(1e-3) < after[k, 2] < F32(20.0), name
        assert after[k, 3] < before[k, 3] or name == "clamped low", (name, after[k], before[k])
    assert after[4, 2] == F32(1e-3) and after[6, 2] == F32(20.0)
    assert after[4, 3] > after[5, 3] + F32(0.05)               # the same v_n on both sides, plus the overshoot on the clamped one
    snap.release()
    ctx.close()


# ---- 3. nothing to do ---------------------------------------------------------------------------------------------------------------
def test_t_zero_leaves_the_snapshot_untouched(B):
    ctx, (mk, mc) = sized_maps(B, 800)
    cur, kf = crafted(B, ctx, mk, mc)
    snap = snapshot_of(mk, kf)
    D = data_of(ctx, snap, cur)
    R, _ = true_motion()
    ref = assert_fusion(B, ctx, mc, snap, D, R, np.zeros(3), "t = 0")
    assert ref["associated"] > 100 and counts_of(ref) == (800, ref["associated"], 0, 0, ref["associated"], 0)
    prs4, mt = snap.download()
    assert prs4.tobytes() == D[1].tobytes() and mt.tobytes() == D[2].tobytes()
    snap.release()
    ctx.close()


def test_an_empty_snapshot_launches_nothing(B):
    ctx, (mk, mc) = sized_maps(B, 0)
    snap = mk.keyframe_snapshot()
    base = B.test_live_resources()
    ctx.profile_reset()
    ctx.profile(True)
    got, assoc = snap.fuse_depth(mc, *true_motion(), want_assoc=True)
    launches = {name: calls for name, (_, calls) in ctx.profile_read().items() if calls}
    ctx.profile(False)
    assert launches == {} and B.test_live_resources() == base, launches
    assert counts_of(got) == (0, 0, 0, 0, 0, 0) and len(assoc) == 0
    snap.release()
    ctx.close()


def test_the_entry_launches_what_it_documents(B):
    """one kernel per call; one allocation at the first call, kept"""
    ctx, (mk, mc) = sized_maps(B, 65)
    cur, kf = crafted(B, ctx, mk, mc)
    snap = snapshot_of(mk, kf)
    snap.download()
    R, t = true_motion()
    base = B.test_live_resources()
    ctx.profile_reset()
    ctx.profile(True)
    snap.fuse_depth(mc, R, t)
    launches = {name: calls for name, (_, calls) in ctx.profile_read().items() if calls}
    assert launches == dict(k_kf_fuse_depth=1), launches
    assert B.test_live_resources() == base + 1
    snap.fuse_depth(mc, R, t, want_assoc=True)
    snap.fuse_depth(mc, R, t)
    launches = {name: calls for name, (_, calls) in ctx.profile_read().items() if calls}
    ctx.profile(False)
    assert launches == dict(k_kf_fuse_depth=3), launches
    assert B.test_live_resources() == base + 1
    snap.release()
    ctx.close()


def test_refusals(B):
    frames, cam = stream()
    live = B.test_live_resources()
    ctx, other = B.Context(params_for(B, cam, **KW_STREAM)), B.Context(params_for(B, cam, **KW_STREAM))
    maps = [ctx.detect_u8(frames[k], k * TS) for k in range(3)]
    foreign = other.detect_u8(frames[0], 0)
    snap, fsnap = maps[0].keyframe_snapshot(), foreign.keyframe_snapshot()
    before = [x.tobytes() for x in snap.download()]
    L = B.lib()
    err = lambda: L.rebvio_hip_last_error().decode()
    out = B.KfFuse()
    dp = C.POINTER(C.c_double)
    R, t = np.eye(3), np.array([0.01, 0.0, 0.0])
    pR, pt = R.ctypes.data_as(dp), t.ctypes.data_as(dp)
    base = B.test_live_resources()
    fuse = L.rebvio_hip_kf_snapshot_fuse_depth
    assert fuse(None, maps[1].h, None, pR, pt, C.byref(out), None) == -3 and "null" in err()
    assert fuse(snap.h, None, None, pR, pt, C.byref(out), None) == -3 and "null" in err()
    assert fuse(snap.h, maps[1].h, None, None, pt, C.byref(out), None) == -3 and "null" in err()
    assert fuse(snap.h, maps[1].h, None, pR, None, C.byref(out), None) == -3 and "null" in err()
    assert fuse(snap.h, maps[1].h, None, pR, pt, None, None) == -3 and "null" in err()
    assert fuse(fsnap.h, maps[1].h, None, pR, pt, C.byref(out), None) == -3 and "another context" in err()
    nan_R = np.eye(3)
    nan_R[2, 0] = np.nan
    sr = int(ctx.p.search_range)
    d = lambda **kw: dict(R=R, t=t, opts=B.default_kf_fuse_opts(ctx, **kw))
    for kw, word in ((dict(R=nan_R, t=t), "non-finite"), (dict(R=R, t=[0.0, 0.0, -np.inf]), "non-finite"), (d(pixel_sigma=0.0), "pixel_sigma"),
                     (d(pixel_sigma=float("nan")), "pixel_sigma"), (d(gate_sigma=0.0), "gate_sigma"), (d(gate_sigma=float("nan")), "gate_sigma"),
                     (d(q_abs=-1.0), "q_abs"), (d(q_abs=float("nan")), "q_abs"), (d(min_cos=1.5), "min_cos"), (d(min_cos=-1.5), "min_cos"),
                     (d(min_cos=float("nan")), "min_cos"), (d(max_dist=-1), "max_dist"), (d(max_dist=sr + 1), "max_dist"), (d(reserved=2), "reserved"),
                     (d(kf_filter=dict(rho_min=-1.0)), "rho_min"), (d(kf_filter=dict(max_rel_sigma=float("nan"))), "NaN")):
        with pytest.raises(B.HipError) as e:
            snap.fuse_depth(maps[1], **kw)
        assert "error -3:" in str(e.value) and word in str(e.value), (kw, str(e.value))
    assert B.test_live_resources() == base                      # nothing was allocated by a refused call
    o = B.default_kf_fuse_opts(ctx)
    assert (o.max_dist, o.pixel_sigma) == (sr, float(ctx.p.pixel_uncertainty))
    # an uploaded map: its field is not detection's - refused
    maps[2].upload(maps[2].keylines())
    with pytest.raises(B.HipError, match="error -7:.*distance field"):
        snap.fuse_depth(maps[2], R, t)
    assert [x.tobytes() for x in snap.download()] == before     # no refused call wrote the snapshot
    snap.fuse_depth(maps[1], R, t, B.default_kf_fuse_opts(ctx, max_dist=sr, min_cos=1.0, q_abs=0.0))      # the bounds themselves are legal
    assert B.test_live_resources() == base + 1
    ctx.close()
    assert fuse(snap.h, maps[1].h, None, pR, pt, C.byref(out), None) == -10 and "destroyed" in err()
    assert fuse(snap.h, foreign.h, None, pR, pt, C.byref(out), None) == -10 and "destroyed" in err()
    snap.release()
    fsnap.release()
    other.close()
    for m in maps + [foreign]:
        m.release()
    assert B.test_live_resources() == live


# ---- 4. with the alignment and the tracker ------------------------------------------------------------------------------------------
def test_the_alignment_sees_the_fused_depths(B):
    """rebvio_hip_map_keyframe_align after a fusion = the restatement's alignment on the restatement's fused snapshot"""
    ctx, (mk, mc) = sized_maps(B, 800)
    cur, kf = crafted(B, ctx, mk, mc)
    snap = snapshot_of(mk, kf)
    R, t = true_motion()
    D = data_of(ctx, snap, cur)
    fused = assert_fusion(B, ctx, mc, snap, D, R, t, "fusion")
    R0, t0 = offset_guess(*OFFSETS[0])
    ref = np_kf_align(D[0], fused["prs4"], fused["matches"], *D[3:], R0, t0)
    stale = np_kf_align(*D, R0, t0)
    assert ref["guard"] > GUARD and stale["guard"] > GUARD
    got, assoc = mc.keyframe_align(snap, None, R0, t0, want_assoc=True)
    d = pose_err(got.R, got.t, ref["R"], ref["t"])
    print(f"alignment after the fusion: err {pose_err(got.R, got.t):.3g} (before it: {pose_err(stale['R'], stale['t']):.3g}) |device - np| {d:.3g} "
          f"used {got.used}")
    assert got.status == ref["status"] == 0 and got.used == ref["used"] and got.iterations == ref["iterations"]
    assert np.array_equal(assoc, ref["assoc"]) and d <= DEV_VS_NP
    assert pose_err(ref["R"], ref["t"], stale["R"], stale["t"]) > 100 * DEV_VS_NP      # the fused depths do change the solve
    snap.release()
    ctx.close()


def test_fusion_calls_between_pairs_disturb_nothing(B):
    """the pair records and the final keylines of the stream are equal word for word with and without alignment and fusion calls
    between the pairs"""
    frames, cam = stream()

    def run(with_fuse):
        ctx = B.Context(params_for(B, cam, **KW_STREAM))
        maps = [ctx.detect_u8(frames[k], k * TS) for k in range(9)]
        recs, snap, R, t = [], None, None, None
        for k in range(8):
            out = ctx.track_pair(maps[k], maps[k + 1])
            recs.append(rec(out, maps[k + 1].size()))
            if k == 1:
                maps[2].mark_keyframe()          # (marked in both runs: the ids are part of what is compared)
                if with_fuse:
                    snap = maps[2].keyframe_snapshot()
                    snap.add_normals(maps[2])
            if k >= 2 and with_fuse:
                got = maps[k + 1].keyframe_align(snap, None, R, t)
                if got.status == 0:
                    R, t = np.array(got.R), np.array(got.t)
                    f = snap.fuse_depth(maps[k + 1], R, t)
                    snap.fuse_depth(maps[k], R, t)              # an older map too
                    print(f"pair {k}: aligned {got.used} of {got.candidates}; fused {counts_of(f)}")
        final = maps[8].keylines()
        if snap:
            snap.release()
        ctx.close()
        return recs, final

    plain, kl_plain = run(False)
    fused, kl_fused = run(True)
    same_records(plain, fused, "with and without alignment and fusion calls")
    assert kl_plain.tobytes() == kl_fused.tobytes()


# ---- the refusal table: every shared refusal with its code and whole text; which one wins when several apply ------

FUSE = "kf_snapshot_fuse_depth"
_fo = lambda s, **kw: s.B.default_kf_fuse_opts(s.ctx, **kw)
_fu = lambda snap, m, s, R="R", t="t", **kw: snap.fuse_depth(m, getattr(s, R) if R else None, getattr(s, t) if t else None, _fo(s, **kw) if kw else None)
REFUSED = {
    "destroyed map": (lambda s: _fu(s.dsnap, s.dm, s), -10, DEAD_MAP),
    "destroyed snapshot": (lambda s: _fu(s.dsnap, s.m, s), -10, DEAD_SNAPSHOT),
    "foreign snapshot": (lambda s: _fu(s.fsnap, s.m, s), -3, foreign_snapshot(FUSE)),
    "no field": (lambda s: _fu(s.snap, s.up, s), -7, no_field(FUSE)),
    "null R": (lambda s: _fu(s.snap, s.m, s, R=None), -3, f"{FUSE}: null R or t"),
    "null t": (lambda s: _fu(s.snap, s.m, s, t=None), -3, f"{FUSE}: null R or t"),
    "R not finite": (lambda s: _fu(s.snap, s.m, s, R="nan_R"), -3, f"{FUSE}: non-finite R or t"),
    "t not finite": (lambda s: _fu(s.snap, s.m, s, t="inf_t"), -3, f"{FUSE}: non-finite R or t"),
    "pixel_sigma": (lambda s: _fu(s.snap, s.m, s, pixel_sigma=0.0), -3, f"{FUSE}: pixel_sigma must be > 0"),
    "gate_sigma": (lambda s: _fu(s.snap, s.m, s, gate_sigma=0.0), -3, f"{FUSE}: gate_sigma must be > 0"),
    "q_abs": (lambda s: _fu(s.snap, s.m, s, q_abs=-1.0), -3, f"{FUSE}: q_abs must be >= 0"),
    "min_cos": (lambda s: _fu(s.snap, s.m, s, min_cos=1.5), -3, f"{FUSE}: min_cos outside [-1, 1]"),
    "max_dist below": (lambda s: _fu(s.snap, s.m, s, max_dist=-1), -3, f"{FUSE}: max_dist outside 0..search_range"),
    "max_dist above": (lambda s: _fu(s.snap, s.m, s, max_dist=s.sr + 1), -3, f"{FUSE}: max_dist outside 0..search_range"),
    "wins: a foreign snapshot over a pose, an option and no field": (lambda s: _fu(s.fsnap, s.up, s, R="nan_R", gate_sigma=0.0), -3,
                                                                     foreign_snapshot(FUSE)),
    "wins: a destroyed snapshot over a null pose": (lambda s: _fu(s.dsnap, s.up, s, R=None), -10, DEAD_SNAPSHOT),
    "wins: a destroyed map over a foreign snapshot": (lambda s: _fu(s.snap, s.dm, s), -10, DEAD_MAP),
    "wins: a null pose over the filter": (lambda s: _fu(s.snap, s.m, s, R=None, kf_filter=dict(rho_min=-1.0)), -3, f"{FUSE}: null R or t"),
    "wins: the filter over the pose": (lambda s: _fu(s.snap, s.m, s, R="nan_R", kf_filter=dict(rho_min=-1.0)), -3,
                                       f"{FUSE}: filter rho_min must be > 0"),
    "wins: the pose over pixel_sigma": (lambda s: _fu(s.snap, s.m, s, R="nan_R", pixel_sigma=0.0), -3, f"{FUSE}: non-finite R or t"),
    "wins: pixel_sigma over gate_sigma": (lambda s: _fu(s.snap, s.m, s, pixel_sigma=0.0, gate_sigma=0.0), -3, f"{FUSE}: pixel_sigma must be > 0"),
    "wins: gate_sigma over q_abs": (lambda s: _fu(s.snap, s.m, s, gate_sigma=0.0, q_abs=-1.0), -3, f"{FUSE}: gate_sigma must be > 0"),
    "wins: q_abs over min_cos": (lambda s: _fu(s.snap, s.m, s, q_abs=-1.0, min_cos=2.0), -3, f"{FUSE}: q_abs must be >= 0"),
    "wins: min_cos over max_dist": (lambda s: _fu(s.snap, s.m, s, min_cos=2.0, max_dist=-1), -3, f"{FUSE}: min_cos outside [-1, 1]"),
    "wins: max_dist over reserved": (lambda s: _fu(s.snap, s.m, s, max_dist=-1, reserved=2), -3, f"{FUSE}: max_dist outside 0..search_range"),
    "wins: an option over no field": (lambda s: _fu(s.snap, s.up, s, reserved=2), -3, f"{FUSE}: reserved must be 0"),
}

@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusal_table(refusal_scene, case):
    """every refusal of the table with its return code and its whole rebvio_hip_last_error text; nothing is allocated"""
    assert_refused(refusal_scene, *REFUSED[case])
