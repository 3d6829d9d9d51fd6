"""numpy restatement of the depth prior (include/rebvio_hip.h, "Depth prior from a registered depth image"), written from the header's
text: float64 behind the loads, one numpy operation per operation of the definition, in its order (numpy fuses nothing). Vectorised
over the keylines; the counts are sums over the outcome words."""
import numpy as np

DEPTH_U16, DEPTH_F32 = 0, 1
RHO_MIN, RHO_MAX = np.float64(np.float32(1e-3)), np.float64(20.0)
DEFAULTS = dict(tap_px=2.0, jump_rel=0.1, z_min=0.1, z_max=20.0, sigma_z0=1e-3, sigma_z2=2e-3, gate_sigma=3.0, q_abs=0.0, unit=0.001)
COUNT_NAMES = ("candidates", "sampled", "fused", "gated", "jumps", "clamped")


def _tap(depth, fmt, x, y, exists, o):
    """z (float64) and validity of one tap per keyline at (x, y)"""
    rows, cols = depth.shape
    with np.errstate(invalid="ignore"):
        xh, yh = x + 0.5, y + 0.5
        inside = exists & (xh >= 0.0) & (xh < cols) & (yh >= 0.0) & (yh < rows)
    xi = np.where(inside, np.floor(np.where(inside, xh, 0.0)), 0.0).astype(np.int64)
    yi = np.where(inside, np.floor(np.where(inside, yh, 0.0)), 0.0).astype(np.int64)
    raw = depth[yi, xi]
    if fmt == DEPTH_U16:
        z = raw.astype(np.float64) * np.float64(o["unit"])
        ok = inside & (raw != 0)
    else:
        z = raw.astype(np.float64)
        ok = inside
    with np.errstate(invalid="ignore"):
        ok = ok & (np.float64(o["z_min"]) <= z) & (z <= np.float64(o["z_max"]))
    return z, ok


def z_near_of(kl, depth, fmt=None, **opts):
    """(z_near, z_far, sampled) per keyline: steps 1 and 2"""
    o = dict(DEFAULTS, **opts)
    depth = np.asarray(depth)
    if fmt is None:
        fmt = DEPTH_U16 if depth.dtype == np.uint16 else DEPTH_F32
    px, py = kl["pos"][:, 0].astype(np.float64), kl["pos"][:, 1].astype(np.float64)
    gn = kl["gradient_norm"].astype(np.float64)
    with np.errstate(all="ignore"):
        ux = kl["gradient"][:, 0].astype(np.float64) / gn
        uy = kl["gradient"][:, 1].astype(np.float64) / gn
        usable = (kl["gradient_norm"] > 0) & np.isfinite(ux) & np.isfinite(uy)
    every = np.ones(len(kl), bool)
    z_near = np.full(len(kl), np.inf)
    z_far = np.full(len(kl), -np.inf)
    sampled = np.zeros(len(kl), bool)
    for s, exists in ((None, every), (1.0, usable), (-1.0, usable)):
        if s is None:
            x, y = px, py
        else:
            d = np.float64(s) * np.float64(o["tap_px"])
            with np.errstate(all="ignore"):
                x, y = px + d * ux, py + d * uy
        z, ok = _tap(depth, fmt, x, y, exists, o)
        z_near = np.where(ok & (z < z_near), z, z_near)
        z_far = np.where(ok & (z > z_far), z, z_far)
        sampled |= ok
    return z_near, z_far, sampled


def depth_prior(kl, depth, fmt=None, **opts):
    """-> (counts dict, updated copy of kl, outcome int32 [n])"""
    o = dict(DEFAULTS, **opts)
    kl = np.array(kl)
    n = len(kl)
    z_near, z_far, sampled = z_near_of(kl, depth, fmt, **opts)
    zn = np.where(sampled, z_near, 1.0)
    zf = np.where(sampled, z_far, 1.0)
    jump = sampled & (zf - zn > np.float64(o["jump_rel"]) * zn)
    rho_m = 1.0 / zn
    s_m = (np.float64(o["sigma_z0"]) * rho_m) * rho_m + np.float64(o["sigma_z2"])
    rho = kl["rho"].astype(np.float64)
    s = kl["sigma_rho"].astype(np.float64)
    q, g = np.float64(o["q_abs"]), np.float64(o["gate_sigma"])
    with np.errstate(all="ignore"):
        v = s * s + q * q
        e = rho_m - rho
        S = v + s_m * s_m
        passed = e * e <= (g * g) * S
        K = v / S
        rho_n = rho + K * e
        v_n = (1.0 - K) * v
        sig_n = np.sqrt(v_n)
        finite = np.isfinite(rho_n) & np.isfinite(v_n) & np.isfinite(sig_n) & (v_n >= 0)
    fused = sampled & passed & finite
    gated = sampled & ~fused
    with np.errstate(all="ignore"):
        low = fused & (rho_n < RHO_MIN)
        high = fused & ~low & (rho_n > RHO_MAX)
        sig_n = np.where(low, sig_n + (RHO_MIN - rho_n), sig_n)
    rho_n = np.where(low, RHO_MIN, np.where(high, RHO_MAX, rho_n))
    clamped = low | high
    with np.errstate(all="ignore"):
        kl["rho"] = np.where(fused, rho_n.astype(np.float32), kl["rho"])
        kl["sigma_rho"] = np.where(fused, sig_n.astype(np.float32), kl["sigma_rho"])
    outcome = (fused * 1 + gated * 2 + jump * 16 + clamped * 32).astype(np.int32)
    counts = dict(candidates=n, sampled=int(sampled.sum()), fused=int(fused.sum()), gated=int(gated.sum()), jumps=int(jump.sum()),
                  clamped=int(clamped.sum()))
    return counts, kl, outcome


def cloud_filter_pass(kl):
    """the default cloud filter (rebvio_hip_default_cloud_filter): matches >= 2, rho in [1e-3, 20], sigma_rho <= 0.5 * rho in fp32"""
    rho, sig = kl["rho"], kl["sigma_rho"]
    with np.errstate(all="ignore"):
        return (kl["matches"] >= 2) & (rho >= np.float32(1e-3)) & (rho <= np.float32(20.0)) & (sig <= np.float32(0.5) * rho)


def oracle_stream(orc_mod, params, frames, depth, with_depth, ts_step=50000):
    """frames through the CPU oracle, keyline sums in the kernels' order; with_depth: depth[k] is fused into map k by the restatement
    (through Map.set_keylines) right after detection for map 0 and after the pair in which k was the new map otherwise. Returns a
    dict: records (PairOut per pair), sizes (the new map's per pair), fusion counts per frame, per frame k >= 1 the median relative
    depth error of the cloud-filter keylines of map k against z_near of depth[k], taken BEFORE that frame's own fusion (NaN where no
    keyline passes), the number that pass, and the newest map's keylines at the end."""
    orc = orc_mod.Oracle(params)
    orc.set_sum_order("device")
    out = dict(records=[], sizes=[], counts=[], err=[np.nan], passing=[0], keylines=None)
    prev = None
    for k in range(len(frames)):
        m = orc.detect_u8(frames[k], k * ts_step)
        if prev is not None:
            out["records"].append(orc.track_pair(prev, m))
            out["sizes"].append(m.size())
            kl = m.keylines()
            z_near, _, sampled = z_near_of(kl, depth[k])
            use = cloud_filter_pass(kl) & sampled
            with np.errstate(all="ignore"):
                rel = np.abs(1.0 / kl["rho"][use].astype(np.float64) - z_near[use]) / z_near[use]
            out["err"].append(float(np.median(rel)) if use.any() else np.nan)
            out["passing"].append(int(use.sum()))
        if with_depth:
            c, kl, _ = depth_prior(m.keylines(), depth[k])
            m.set_keylines(kl)
            out["counts"].append(c)
        prev = m
    out["keylines"] = prev.keylines()
    return out


def counts_tuple(c):
    return tuple(int(c[k]) if isinstance(c, dict) else int(getattr(c, k)) for k in COUNT_NAMES)
