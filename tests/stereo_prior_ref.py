"""numpy restatement of the stereo prior (include/rebvio_hip.h, "Depth prior from a rectified stereo partner"), written from the
header's text: float64 behind the loads, one numpy operation per operation of the definition, in its order (numpy fuses nothing).
Vectorised over the left keylines, one pass per cell offset of the window; the counts are sums over the outcome words."""
import math

import numpy as np

from depth_prior_ref import cloud_filter_pass, z_near_of

RHO_MIN, RHO_MAX = np.float64(np.float32(1e-3)), np.float64(20.0)
COS45 = float(np.float32(math.cos(45.0 * math.pi / 180.0)))
DEFAULTS = dict(d_min=0.0, d_max=64.0, min_ux=0.5, row_tol=1, sigma_px=0.5, gate_sigma=3.0, ambig_px=2.0, cos_min=COS45, norm_tol=1.0,
                q_abs=0.0)
COUNT_NAMES = ("candidates", "usable", "seen", "fused", "gated", "ambiguous", "clamped", "reserved")
NONE, FUSED, GATED, UNUSABLE, AMBIGUOUS, CLAMPED = 0, 1, 2, 3, 4, 32


def stereo_prior(left, right, right_mask, rows, cols, fm, **opts):
    """-> (counts dict, updated copy of left, outcome int32 [n], winner int32 [n]); opts must hold baseline"""
    o = dict(DEFAULTS, **opts)
    f8 = np.float64
    kl = np.array(left)
    n, nr = len(kl), len(right)
    mask = np.asarray(right_mask, np.int32).reshape(rows, cols)
    fb = f8(np.float32(fm)) * f8(o["baseline"])
    px, py = kl["pos"][:, 0].astype(f8), kl["pos"][:, 1].astype(f8)
    gx, gy, gn = kl["gradient"][:, 0].astype(f8), kl["gradient"][:, 1].astype(f8), kl["gradient_norm"].astype(f8)
    rho, s = kl["rho"].astype(f8), kl["sigma_rho"].astype(f8)
    with np.errstate(all="ignore"):
        # 1
        ux, uy = gx / gn, gy / gn
        usable = (kl["gradient_norm"] > 0) & np.isfinite(ux) & np.isfinite(uy) & (np.abs(ux) >= f8(o["min_ux"]))
        # 2
        xh, yh = px + 0.5, py + 0.5
        inside = usable & (xh >= 0.0) & (xh < cols) & (yh >= 0.0) & (yh < rows)
        xi = np.floor(np.where(inside, xh, 0.0)).astype(np.int64)
        yi = np.floor(np.where(inside, yh, 0.0)).astype(np.int64)
        # 4, the keyline's own part
        v = s * s + f8(o["q_abs"]) * f8(o["q_abs"])
        s_m = (f8(o["sigma_px"]) / np.abs(ux)) / fb
        S = v + s_m * s_m
    g2 = f8(o["gate_sigma"]) * f8(o["gate_sigma"])
    seen = np.zeros(n, bool)
    gate = np.zeros(n, bool)
    d_lo, d_hi = np.full(n, np.inf), np.full(n, -np.inf)
    best, best_j, best_d = np.full(n, np.inf), np.full(n, np.iinfo(np.int64).max), np.zeros(n)
    first, last = -(int(math.ceil(o["d_max"])) + 1), -(int(math.floor(o["d_min"])) - 1)
    for dy in ((0, -1, 1) if o["row_tol"] else (0,)):
        y = yi + dy
        row_ok = inside & (y >= 0) & (y < rows)
        for off in range(first, last + 1):
            x = xi + off
            ok = row_ok & (x >= 0) & (x < cols)
            j = mask[np.where(ok, y, 0), np.where(ok, x, 0)].astype(np.int64)
            ok &= (j >= 0) & (j < nr)
            if not ok.any():
                continue
            jj = np.where(ok, j, 0)
            qx, qy = right["pos"][jj, 0].astype(f8), right["pos"][jj, 1].astype(f8)
            hx, hy, hn = right["gradient"][jj, 0].astype(f8), right["gradient"][jj, 1].astype(f8), right["gradient_norm"][jj].astype(f8)
            with np.errstate(all="ignore"):
                # 3
                ok &= hn > 0.0
                ok &= (gx * hx + gy * hy) / (gn * hn) >= f8(o["cos_min"])
                ok &= np.abs(hn / gn - 1.0) <= f8(o["norm_tol"])
                uxr, uyr = hx / hn, hy / hn
                ok &= np.abs(uxr) >= f8(o["min_ux"])
                xr = qx - (uyr * (py - qy)) / uxr
                d = px - xr
                ok &= (d > 0.0) & (f8(o["d_min"]) <= d) & (d <= f8(o["d_max"]))
                # 4
                rho_m = d / fb
                e = rho_m - rho
                ing = ok & (e * e <= g2 * S)
                ex, ey = gx - hx, gy - hy
                score = ex * ex + ey * ey
            seen |= ok
            gate |= ing
            d_lo = np.where(ing & (d < d_lo), d, d_lo)
            d_hi = np.where(ing & (d > d_hi), d, d_hi)
            better = ing & ((score < best) | ((score == best) & (jj < best_j)))
            best = np.where(better, score, best)
            best_j = np.where(better, jj, best_j)
            best_d = np.where(better, d, best_d)
    with np.errstate(all="ignore"):
        # 5
        ambiguous = gate & (d_hi - d_lo > f8(o["ambig_px"]))
        # 6
        won = gate & ~ambiguous
        rho_m = best_d / fb
        e = rho_m - rho
        K = v / S
        rho_n = rho + K * e
        v_n = (1.0 - K) * v
        sig_n = np.sqrt(v_n)
        finite = np.isfinite(rho_n) & np.isfinite(v_n) & np.isfinite(sig_n) & (v_n >= 0)
        fused = won & finite
        low = fused & (rho_n < RHO_MIN)
        high = fused & ~low & (rho_n > RHO_MAX)
        sig_n = np.where(low, sig_n + (RHO_MIN - rho_n), sig_n)
        rho_n = np.where(low, RHO_MIN, np.where(high, RHO_MAX, rho_n))
        kl["rho"] = np.where(fused, rho_n.astype(np.float32), kl["rho"])
        kl["sigma_rho"] = np.where(fused, sig_n.astype(np.float32), kl["sigma_rho"])
    gated = (seen & ~gate) | (won & ~finite)
    clamped = low | high
    outcome = np.where(~usable, UNUSABLE, fused * FUSED + gated * GATED + ambiguous * AMBIGUOUS + clamped * CLAMPED).astype(np.int32)
    winner = np.where(fused, best_j, -1).astype(np.int32)
    counts = dict(candidates=n, usable=int(usable.sum()), seen=int(seen.sum()), fused=int(fused.sum()), gated=int(gated.sum()),
                  ambiguous=int(ambiguous.sum()), clamped=int(clamped.sum()), reserved=0)
    return counts, kl, outcome, winner


def counts_tuple(c):
    return tuple(int(c[k]) if isinstance(c, dict) else int(getattr(c, k)) for k in COUNT_NAMES)


def oracle_stream(orc_mod, params, left, right, baseline, depth=None, ts_step=50000, opts=None):
    """The left frames through the CPU oracle, keyline sums in the kernels' order. right = None: no stereo. Otherwise a second,
    detect-only oracle detects right[k], and the restatement fuses its map into left map k (through Map.set_keylines) right after
    detection for map 0 and after the pair in which k was the new map otherwise. Returns a dict: records (PairOut per pair), sizes
    (the new map's per pair), fusion counts and outcome words per frame, every left map's keylines before and after its fusion, every
    right map's (keylines, mask), and - with the
    rendered depth images - per frame k >= 1 the median relative depth error of the cloud-filter keylines of map k against z_near of
    depth[k], taken BEFORE that frame's own fusion (NaN where no keyline passes), and the number that pass."""
    rows, cols = params.rows, params.cols
    orc = orc_mod.Oracle(params)
    orc.set_sum_order("device")
    orc_r = orc_mod.Oracle(params) if right is not None else None
    out = dict(records=[], sizes=[], counts=[], outcomes=[], err=[np.nan], passing=[0], keylines=[], right=[], before=[])
    prev = None
    for k in range(len(left)):
        m = orc.detect_u8(left[k], k * ts_step)
        if prev is not None:
            out["records"].append(orc.track_pair(prev, m))
            out["sizes"].append(m.size())
            if depth is not None:
                kl = m.keylines()
                z_near, _, sampled = z_near_of(kl, depth[k])
                use = cloud_filter_pass(kl) & sampled
                with np.errstate(all="ignore"):
                    rel = np.abs(1.0 / kl["rho"][use].astype(np.float64) - z_near[use]) / z_near[use]
                out["err"].append(float(np.median(rel)) if use.any() else np.nan)
                out["passing"].append(int(use.sum()))
        if right is not None:
            mr = orc_r.detect_u8(right[k], k * ts_step)
            kr, mask_r = mr.keylines(), mr.mask(rows, cols)
            out["before"].append(m.keylines())
            c, kl, oc, _ = stereo_prior(out["before"][-1], kr, mask_r, rows, cols, params.fm, baseline=baseline, **(opts or {}))
            m.set_keylines(kl)
            out["counts"].append(c)
            out["outcomes"].append(oc)
            out["right"].append((kr, mask_r))
        out["keylines"].append(m.keylines())
        prev = m
    return out
