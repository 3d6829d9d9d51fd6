"""The depth fusion of a map into a keyframe snapshot (rebvio_hip_kf_snapshot_fuse_depth) restated in numpy float64, expression by
expression after the comment in include/rebvio_hip.h, on top of the alignment's lookup and residual (kf_align_ref._lookup /
_residual). A plain helper module like support.py and kf_align_ref.py: no test lives here and importing it needs no GPU."""
import numpy as np

from kf_align_ref import _lookup, _residual
from kf_pose_ref import DEFAULT_FILTER
from support import F32, np_passes

INT_MIN = -2 ** 31
RHO_MIN = np.float64(F32(1e-3))      # the constants the tracker clamps to (types/keyline.hpp), as doubles of the floats
RHO_MAX = np.float64(F32(20.0))
COUNTS = ("candidates", "associated", "fused", "gated", "flat", "clamped")


def np_kf_fuse(cam, prs4, kf_matches, normals, cur_pos, cur_unit, ids, dists, R, t, flt=DEFAULT_FILTER, min_cos=0.9, max_dist=40,
               pixel_sigma=1.0, gate_sigma=3.0, q_abs=0.0):
    """One fusion at (R, t). Returns dict(prs4, matches: the snapshot afterwards (new arrays); assoc int32 [n]; the six counts;
    e, h, K: the residual, de/drho and the gain per keyline (NaN where not associated); guards). guards - the smallest distance of
    any keyline from a decision two implementations could take differently: `edge` (px, of a projection from a cell edge), `gate`
    (of the min_cos test from its switch), `innov` (of e * e from the innovation bound, relative to the bound), `info` (of info from
    0, relative to the two addends it is made of: 1 unless it underflows), `clamp` (of rho_n from RHO_MIN and RHO_MAX)."""
    fm, cx, cy, rows, cols = cam
    prs4 = np.array(prs4, F32).reshape(-1, 4)
    mt = np.array(kf_matches, np.uint32).reshape(-1)
    n = len(prs4)
    pos = np.asarray(cur_pos, F32).reshape(-1, 2)
    unit = np.asarray(cur_unit, F32).reshape(-1, 2)
    R9 = np.asarray(R, np.float64).reshape(9)
    t3 = np.asarray(t, np.float64).reshape(3)
    out = dict(prs4=prs4, matches=mt, assoc=np.full(n, INT_MIN, np.int32), candidates=n, associated=0, fused=0, gated=0, flat=0, clamped=0,
               e=np.full(n, np.nan), h=np.full(n, np.nan), K=np.full(n, np.nan),
               guards=dict(edge=np.inf, gate=np.inf, innov=np.inf, info=np.inf, clamp=np.inf))
    if n == 0 or len(pos) == 0:
        return out
    # 1. the filter, then steps 2..5 of the alignment (the lookup) and step 6's own skips
    kf = np.zeros(n, np.dtype([("rho", "<f4"), ("sigma_rho", "<f4"), ("matches", "<u4")]))
    kf["rho"], kf["sigma_rho"], kf["matches"] = prs4[:, 2], prs4[:, 3], mt
    with np.errstate(all="ignore"):
        passed = np_passes(kf, *flt)
        ok, i, g = _lookup(cam, prs4, normals, pos, unit, ids, dists, R9, t3, min_cos, max_dist)
        q = (pos - np.array([F32(cx), F32(cy)], F32)).astype(F32)       # pos - (cx, cy): fp32 subtractions
        un = unit[i].astype(np.float64)
        g2 = un[:, 0] * un[:, 0] + un[:, 1] * un[:, 1]
        ok = ok & passed & (g2 > 0) & (g2 < np.inf)
        # 2. e and c of the pose term
        f32fm = F32(fm)
        a = (prs4[:, 0] / f32fm).astype(F32).astype(np.float64)
        b = (prs4[:, 1] / f32fm).astype(F32).astype(np.float64)
        rho = prs4[:, 2].astype(np.float64)
        Z = [(R9[3 * r] * a + R9[3 * r + 1] * b) + R9[3 * r + 2] for r in range(3)]
        Y = [Z[r] + rho * t3[r] for r in range(3)]
        px, py = Y[0] / Y[2], Y[1] / Y[2]
        gn = np.sqrt(g2)
        nx, ny = un[:, 0] / gn, un[:, 1] / gn
        f = np.float64(f32fm)
        e = _residual(fm, prs4, q, unit, i, R9, t3)
        ccx, ccy = (f * nx) / Y[2], (f * ny) / Y[2]
        ccz = -(ccx * px + ccy * py)
        # 3..6
        h = (ccx * t3[0] + ccy * t3[1]) + ccz * t3[2]
        s = prs4[:, 3].astype(np.float64)
        v = s * s + q_abs * q_abs
        hv = h * v
        info = hv * h
        flat = ok & ~(info > 0)
        S = info + pixel_sigma * pixel_sigma
        bound = (gate_sigma * gate_sigma) * S
        live = ok & ~flat
        gated = live & ~(e * e <= bound)
        K = hv / S
        rho_n = rho - K * e
        v_n = (1.0 - K * h) * v
        sig_n = np.sqrt(v_n)
        fine = np.isfinite(rho_n) & np.isfinite(v_n) & np.isfinite(sig_n) & (v_n >= 0)
        gated |= live & ~fine
        fused = live & ~gated
        # 7. the clamps
        low = fused & (rho_n < RHO_MIN)
        high = fused & ~low & (rho_n > RHO_MAX)
        sig_c = np.where(low, sig_n + (RHO_MIN - rho_n), sig_n)
        rho_c = np.where(low, RHO_MIN, np.where(high, RHO_MAX, rho_n))
        # 8.
        prs4[fused, 2] = rho_c[fused].astype(F32)
        prs4[fused, 3] = sig_c[fused].astype(F32)
        mt[fused & (mt != 0xFFFFFFFF)] += np.uint32(1)
        # guards
        rel = lambda x, y: np.abs(x) / np.where(y > 0, y, 1.0)
        gd = out["guards"]
        gd["edge"] = float(g["edge"][passed].min()) if passed.any() else np.inf
        gd["gate"] = float(g["gate"][passed].min()) if passed.any() else np.inf
        if ok.any():
            scale = (np.abs(ccx * t3[0]) + np.abs(ccy * t3[1])) + np.abs(ccz * t3[2])
            d = np.where(np.isfinite(h) & (scale > 0) & (v > 0), rel(h, scale), np.inf)      # (all addends 0, or v 0 or NaN: no choice to take)
            gd["info"] = float(d[ok].min())
        if live.any():
            d = rel(e[live] * e[live] - bound[live], bound[live])
            gd["innov"] = float(np.where(np.isfinite(d), d, np.inf).min())
        if (live & fine).any():
            m = live & fine & ~gated
            if m.any():
                gd["clamp"] = float(np.minimum(np.abs(rho_n[m] - RHO_MIN), np.abs(rho_n[m] - RHO_MAX)).min())
    out["assoc"] = np.where(fused, i, np.where(ok, -1 - i, INT_MIN)).astype(np.int32)
    out.update(associated=int(ok.sum()), fused=int(fused.sum()), gated=int(gated.sum()), flat=int(flat.sum()), clamped=int((low | high).sum()))
    out["e"], out["h"], out["K"] = np.where(ok, e, np.nan), np.where(ok, h, np.nan), np.where(fused, K, np.nan)
    return out


def counts_of(x):
    """the six counts of a restatement's dict or of a KfFuse struct, as a tuple"""
    if isinstance(x, dict):
        return tuple(int(x[k]) for k in COUNTS)
    return tuple(int(getattr(x, k)) for k in COUNTS)


def perturbed(craft, seed, scale=1.0):
    """the crafted keyframe keylines (kf_align_ref.craft_against) with rho moved by a seeded normal draw of its own sigma_rho x scale,
    clipped to 2.5 sigma: (prs4 with the perturbed rho, rho_true float64)"""
    rng = np.random.default_rng(seed)
    prs4 = np.array(craft["prs4"], F32)
    rho_true = prs4[:, 2].astype(np.float64)
    z = np.clip(rng.standard_normal(len(prs4)), -2.5, 2.5)
    prs4[:, 2] = (rho_true + scale * z * prs4[:, 3].astype(np.float64)).astype(F32)
    return prs4, rho_true


def nees(prs4, rho_true, mask):
    """sum over mask of (rho - rho_true)^2 / sigma_rho^2, in float64"""
    p = np.asarray(prs4, F32).reshape(-1, 4).astype(np.float64)
    return float((((p[:, 2] - rho_true) ** 2) / (p[:, 3] ** 2))[mask].sum())
