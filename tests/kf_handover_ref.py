"""The depth hand-over from a retiring keyframe snapshot to its successor (rebvio_hip_kf_snapshot_handover_depth) restated in numpy
float64, expression by expression after the comment in include/rebvio_hip.h, on top of the alignment's lookup
(kf_align_ref._lookup), and the crafted inputs the hand-over tests share. A plain helper module like support.py and kf_fuse_ref.py:
no test lives here and importing it needs no GPU."""
import numpy as np

from kf_align_ref import _lookup
from kf_fuse_ref import INT_MIN, RHO_MAX, RHO_MIN
from kf_pose_ref import DEFAULT_FILTER
from support import F32, np_passes

COUNTS = ("candidates", "associated", "out_of_range", "claimed", "adopted", "kept", "conflicts")


def np_kf_handover(cam, prs4, kf_matches, normals, cur_pos, cur_unit, ids, dists, dst_prs4, dst_matches, R, t, flt=DEFAULT_FILTER,
                   min_cos=0.9, max_dist=40, gate_sigma=3.0, q_abs=0.0):
    """One hand-over at (R, t). Returns dict(prs4, matches: dst afterwards (new arrays); assoc int32 [n]; the seven counts; rho_c,
    sig_c, d: the propagated pair and d rho_c / d rho per src keyline in float64 (NaN where not associated); winner int64 [m]: the
    winning j per dst slot, -1 where unclaimed; guards). guards - the smallest distance of anything from a decision two
    implementations could take differently: `edge` (px, of a projection from a cell edge), `gate` (of the min_cos test from its
    switch), `range` (of rho_c from RHO_MIN and RHO_MAX), `conflict` (of dr * dr from the conflict bound, relative to the bound).
    Ties in sigma and sc < sigma_i compare identical fp32 bits and have no guard."""
    fm, cx, cy, rows, cols = cam
    prs4 = np.asarray(prs4, F32).reshape(-1, 4)
    mt = np.asarray(kf_matches, np.uint32).reshape(-1)
    dp = np.array(dst_prs4, F32).reshape(-1, 4)
    dm = np.array(dst_matches, np.uint32).reshape(-1)
    n, m = len(prs4), len(dp)
    pos = np.asarray(cur_pos, F32).reshape(-1, 2)
    unit = np.asarray(cur_unit, F32).reshape(-1, 2)
    R9 = np.asarray(R, np.float64).reshape(9)
    t3 = np.asarray(t, np.float64).reshape(3)
    out = dict(prs4=dp, matches=dm, assoc=np.full(n, INT_MIN, np.int32), candidates=n, associated=0, out_of_range=0, claimed=0, adopted=0,
               kept=0, conflicts=0, rho_c=np.full(n, np.nan), sig_c=np.full(n, np.nan), d=np.full(n, np.nan), winner=np.full(m, -1, np.int64),
               guards=dict(edge=np.inf, gate=np.inf, range=np.inf, conflict=np.inf))
    if n == 0 or len(pos) == 0:
        return out
    kf = np.zeros(n, np.dtype([("rho", "<f4"), ("sigma_rho", "<f4"), ("matches", "<u4")]))
    kf["rho"], kf["sigma_rho"], kf["matches"] = prs4[:, 2], prs4[:, 3], mt
    with np.errstate(all="ignore"):
        # 1. the filter, steps 2..5 of the alignment (the lookup), step 6's own skip, the owner below dst's size
        passed = np_passes(kf, *flt)
        ok, i, g = _lookup(cam, prs4, normals, pos, unit, ids, dists, R9, t3, min_cos, max_dist)
        un = unit[i].astype(np.float64)
        g2 = un[:, 0] * un[:, 0] + un[:, 1] * un[:, 1]
        ok = ok & passed & (g2 > 0) & (g2 < np.inf) & (i < m)
        # 2. propagate
        f32fm = F32(fm)
        a = (prs4[:, 0] / f32fm).astype(F32).astype(np.float64)
        b = (prs4[:, 1] / f32fm).astype(F32).astype(np.float64)
        rho = prs4[:, 2].astype(np.float64)
        Zz = (R9[6] * a + R9[7] * b) + R9[8]
        Yz = Zz + rho * t3[2]
        rho_c = rho / Yz
        d = Zz / (Yz * Yz)
        s = prs4[:, 3].astype(np.float64)
        sig_c = np.abs(d) * np.sqrt(s * s + q_abs * q_abs)
        inr = np.isfinite(rho_c) & np.isfinite(sig_c) & (sig_c >= 0) & (rho_c >= RHO_MIN) & (rho_c <= RHO_MAX)
        claim = ok & inr
        rc32, sc32 = rho_c.astype(F32), sig_c.astype(F32)
    # 3. the claims: the smallest (bits of sc32, j) per owner
    keys = (sc32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    best = np.full(m, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    np.minimum.at(best, i[claim], keys[claim])
    claimed = best != np.uint64(0xFFFFFFFFFFFFFFFF)
    win = np.where(claimed, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), 0)
    # 4..5 per claimed slot
    with np.errstate(all="ignore"):
        rc, sc = rc32[win], sc32[win]
        dr = rc.astype(np.float64) - dp[:, 2].astype(np.float64)
        bound = (gate_sigma * gate_sigma) * (sc.astype(np.float64) * sc.astype(np.float64) + dp[:, 3].astype(np.float64) * dp[:, 3].astype(np.float64))
        agree = claimed & (dr * dr <= bound)
        conflict = claimed & ~agree
        adopted = agree & (sc < dp[:, 3])
        kept = agree & ~adopted
        rel = np.abs(dr * dr - bound) / np.where(bound > 0, bound, 1.0)
    sl = np.flatnonzero(adopted)
    dp[sl, 2], dp[sl, 3] = rc[sl], sc[sl]
    dm[sl] = np.maximum(dm[sl], mt[win[sl]])
    assoc = np.where(ok, -1 - i, INT_MIN).astype(np.int64)
    assoc[win[sl]] = sl
    gd = out["guards"]
    gd["edge"] = float(g["edge"][passed].min()) if passed.any() else np.inf
    gd["gate"] = float(g["gate"][passed].min()) if passed.any() else np.inf
    fin = ok & np.isfinite(rho_c)
    if fin.any():
        gd["range"] = float(np.minimum(np.abs(rho_c[fin] - RHO_MIN), np.abs(rho_c[fin] - RHO_MAX)).min())
    if claimed.any():
        r = rel[claimed]
        gd["conflict"] = float(np.where(np.isfinite(r), r, np.inf).min())
    out.update(assoc=assoc.astype(np.int32), associated=int(ok.sum()), out_of_range=int((ok & ~inr).sum()), claimed=int(claimed.sum()),
               adopted=int(adopted.sum()), kept=int(kept.sum()), conflicts=int(conflict.sum()), rho_c=np.where(ok, rho_c, np.nan),
               sig_c=np.where(ok, sig_c, np.nan), d=np.where(ok, d, np.nan), winner=np.where(claimed, win, -1))
    return out


def counts_of(x):
    """the seven counts of a restatement's dict or of a KfHandover struct, as a tuple"""
    if isinstance(x, dict):
        return tuple(int(x[k]) for k in COUNTS)
    return tuple(int(getattr(x, k)) for k in COUNTS)


def assert_identities(c):
    """the bookkeeping identities on a counts tuple"""
    cand, assoc, oor, claimed, adopted, kept, conf = c
    assert claimed == adopted + kept + conf and assoc - oor - claimed >= 0 and assoc <= cand, c


def guard_min(ref):
    return min(ref["guards"].values())


def smooth_rho(pos, cam):
    """the inverse depth of a smooth scene at pixel positions pos [n, 2]: a tilted, gently curved surface, rho in [0.4, 1.6]"""
    fm, cx, cy, rows, cols = cam
    u = (np.asarray(pos, np.float64)[:, 0] - cx) / cols
    v = (np.asarray(pos, np.float64)[:, 1] - cy) / rows
    return 1.0 + 0.45 * u - 0.3 * v + 0.25 * np.sin(3.0 * u) * np.cos(2.0 * v)


def purpose_case(scene, seed, dst_rel=0.2, src_rel=0.05, clip=2.5):
    """The purpose test's inputs on an oracle scene (kf_align_ref.oracle_scene): every keyline i of the map takes rho_true[i] from
    smooth_rho at its pos. dst [n_map] carries it perturbed by a seeded draw at sigma = dst_rel * rho_true, clipped at `clip`
    sigmas, matches 1. src is crafted behind the true motion (kf_pose_ref.true_motion) for every keyline that owns its own cell, as
    kf_align_ref.craft_against does, from the same rho_true, with sigma = src_rel * rho_kf and perturbed by its own sigma (its own
    seeded draw, clipped). Returns dict(src_prs4, src_matches, src_normals, owner, dst_prs4, dst_matches, rho_true)."""
    from kf_pose_ref import true_motion
    fm, cx, cy, rows, cols = scene["cam"]
    rng = np.random.default_rng(seed)
    pos = np.asarray(scene["pos"], F32).reshape(-1, 2).astype(np.float64)
    nmap = len(pos)
    rho_true = smooth_rho(pos, (np.float64(F32(fm)), np.float64(F32(cx)), np.float64(F32(cy)), rows, cols))
    z = np.clip(rng.standard_normal(nmap), -clip, clip)
    dst = np.zeros((nmap, 4), F32)
    dst[:, 0], dst[:, 1] = (pos[:, 0] - np.float64(F32(cx))).astype(F32), (pos[:, 1] - np.float64(F32(cy))).astype(F32)
    dst[:, 3] = (dst_rel * rho_true).astype(F32)
    dst[:, 2] = (rho_true + z * dst[:, 3].astype(np.float64)).astype(F32)
    ids = np.asarray(scene["ids"]).reshape(rows, cols)
    dists = np.asarray(scene["dists"]).reshape(rows, cols)
    x, y = np.floor(pos[:, 0] + 0.5).astype(np.int64), np.floor(pos[:, 1] + 0.5).astype(np.int64)
    inside = (x >= 1) & (x <= cols - 2) & (y >= 1) & (y <= rows - 2)
    xc, yc = np.clip(x, 0, cols - 1), np.clip(y, 0, rows - 1)
    unit = np.asarray(scene["unit"], F32).astype(np.float64)
    owner = np.flatnonzero(inside & (ids[yc, xc] == np.arange(nmap)) & (dists[yc, xc] == 0) & ((unit ** 2).sum(1) > 0))
    n = len(owner)
    R, t = true_motion()
    ray = np.stack([(pos[owner, 0] - np.float64(F32(cx))) / np.float64(F32(fm)), (pos[owner, 1] - np.float64(F32(cy))) / np.float64(F32(fm)),
                    np.ones(n)], 1)
    X_kf = (ray / rho_true[owner][:, None] - t) @ R
    assert (X_kf[:, 2] > 0.2).all()
    kf_pos = np.float64(F32(fm)) * X_kf[:, :2] / X_kf[:, 2:3]
    nrm = unit[owner] @ R[:2, :2]
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    rho_kf = 1.0 / X_kf[:, 2]
    sig = (src_rel * rho_kf).astype(F32)
    zs = np.clip(rng.standard_normal(n), -clip, clip)
    src = np.concatenate([kf_pos.astype(F32), (rho_kf + zs * sig.astype(np.float64)).astype(F32)[:, None], sig[:, None]], 1).astype(F32)
    return dict(src_prs4=src, src_matches=np.full(n, 3, np.uint32), src_normals=nrm.astype(F32), owner=owner, dst_prs4=dst,
                dst_matches=np.ones(nmap, np.uint32), rho_true=rho_true)
