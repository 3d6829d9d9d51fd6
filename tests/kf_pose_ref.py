"""The keyframe-to-current pose (rebvio_hip_map_keyframe_pose) restated in numpy float64, expression by expression after the comment
in include/rebvio_hip.h, and the crafted inputs the pose tests share. A plain helper module like support.py: no test lives here and
importing it needs no GPU."""
import numpy as np

from support import F32, KF_MATCH_DTYPE, np_passes, rodrigues

N_SUMS = 28
DEFAULT_FILTER = (2, 0.5, 1e-3, 20.0)     # rebvio_hip_default_cloud_filter: min_matches, max_rel_sigma, rho_min, rho_max
W_TRUE = (0.03, -0.05, 0.04)              # the crafted motion: R = exp(W_TRUE), t = T_TRUE
T_TRUE = (0.08, -0.05, 0.1)


def true_motion():
    return rodrigues(W_TRUE), np.array(T_TRUE, np.float64)


def pose_err(R, t, R_ref=None, t_ref=None):
    """max-abs distance over R and t, from the crafted motion unless another pose is given"""
    if R_ref is None:
        R_ref, t_ref = true_motion()
    return max(np.abs(np.asarray(R, np.float64).reshape(3, 3) - np.asarray(R_ref).reshape(3, 3)).max(),
               np.abs(np.asarray(t, np.float64).reshape(3) - np.asarray(t_ref).reshape(3)).max())


def _terms(fm, prs4, kf_matches, cur_pos_img, cur_grad, records, R, t, flt, huber):
    """(used mask over the records, terms [n_rec, 28] with the unused rows zero)"""
    fm = F32(fm)
    R = np.asarray(R, np.float64).reshape(9)
    t = np.asarray(t, np.float64).reshape(3)
    j, i = records["kf_keyline"].astype(np.int64), records["keyline"].astype(np.int64)
    prs4 = np.asarray(prs4, F32).reshape(-1, 4)
    k = prs4[j]
    with np.errstate(all="ignore"):
        kf = np.zeros(len(j), np.dtype([("rho", "<f4"), ("sigma_rho", "<f4"), ("matches", "<u4")]))
        kf["rho"], kf["sigma_rho"], kf["matches"] = k[:, 2], k[:, 3], np.asarray(kf_matches, np.uint32)[j]
        ok = np_passes(kf, *flt)
        a = (k[:, 0] / fm).astype(F32).astype(np.float64)
        b = (k[:, 1] / fm).astype(F32).astype(np.float64)
        rho = k[:, 2].astype(np.float64)
        q = np.asarray(cur_pos_img, F32).reshape(-1, 2)[i]
        qx = (q[:, 0] / fm).astype(F32).astype(np.float64)
        qy = (q[:, 1] / fm).astype(F32).astype(np.float64)
        g = np.asarray(cur_grad, F32).reshape(-1, 2)[i].astype(np.float64)
        gx, gy = g[:, 0], g[:, 1]
        g2 = gx * gx + gy * gy
        ok &= (g2 > 0) & (g2 < np.inf)
        gn = np.sqrt(g2)
        nx, ny = gx / gn, gy / gn
        Z = [(R[3 * r] * a + R[3 * r + 1] * b) + R[3 * r + 2] for r in range(3)]
        Y = [Z[r] + rho * t[r] for r in range(3)]
        ok &= Y[2] > 0
        px, py = Y[0] / Y[2], Y[1] / Y[2]
        f = np.float64(fm)
        e = f * (nx * (px - qx) + ny * (py - qy))
        cx, cy = (f * nx) / Y[2], (f * ny) / Y[2]
        cz = -(cx * px + cy * py)
        J = [rho * cx, rho * cy, rho * cz, Z[1] * cz - Z[2] * cy, Z[2] * cx - Z[0] * cz, Z[0] * cy - Z[1] * cx]
        ae = np.abs(e)
        inside = ae <= huber
        w = np.where(inside, 1.0, huber / ae)
        cols = []
        for r in range(6):
            wj = w * J[r]
            cols.extend(wj * J[c] for c in range(r, 6))
        for r in range(6):
            cols.append((w * J[r]) * e)
        cols.append(np.where(inside, (e * e) / 2.0, huber * (ae - huber / 2.0)))
    # H entries come first, row by row; then g; then the cost: the order of the library's 28 sums
    H = cols[:21]
    order = H + cols[21:27] + [cols[27]]
    terms = np.stack(order, 1) if len(j) else np.zeros((0, N_SUMS))
    terms[~ok] = 0.0
    return ok, terms


def np_kf_pose_sums(fm, prs4, kf_matches, cur_pos_img, cur_grad, records, R, t, flt=DEFAULT_FILTER, huber=2.0):
    """The 28 sums at (R, t): (sums [28]: the 21 H(a, b), a <= b, row by row, the 6 g, the cost; sum of |term| per sum [28]; used)"""
    ok, terms = _terms(fm, prs4, kf_matches, cur_pos_img, cur_grad, records, R, t, flt, huber)
    return terms.sum(0), np.abs(terms).sum(0), int(ok.sum())


def unpack_sums(S):
    """(H [6, 6], g [6], cost) of 28 sums"""
    H = np.zeros((6, 6))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            H[a, b] = H[b, a] = S[k]
            k += 1
    return H, np.array(S[21:27]), float(S[27])


def pose_sums(p):
    """the 28 sums of a KfPose result (its H is the full symmetric matrix)"""
    H = np.array(p.H, np.float64).reshape(6, 6)
    return np.concatenate([[H[a, b] for a in range(6) for b in range(a, 6)], np.array(p.g, np.float64), [p.cost]])


def np_kf_pose(fm, prs4, kf_matches, cur_pos_img, cur_grad, records, R0=None, t0=None, flt=DEFAULT_FILTER, huber=2.0, max_iter=8,
               min_used=12):
    """The whole solve: max_iter + 1 evaluations, a Cholesky step behind every one but the last. Returns a dict with the fields of
    rebvio_hip_kf_pose."""
    R = np.eye(3) if R0 is None else np.array(R0, np.float64).reshape(3, 3)
    t = np.zeros(3) if t0 is None else np.array(t0, np.float64).reshape(3)
    status = iterations = 0
    for it in range(max_iter + 1):
        S, _, used = np_kf_pose_sums(fm, prs4, kf_matches, cur_pos_img, cur_grad, records, R, t, flt, huber)
        H, g, cost = unpack_sums(S)
        if it == 0 and used < min_used:
            status = 3
        if it == max_iter or status != 0:
            continue
        try:
            L = np.linalg.cholesky(H)
            if not np.isfinite(L).all():
                raise np.linalg.LinAlgError
        except np.linalg.LinAlgError:
            status = 2
            continue
        d = np.linalg.solve(L.T, np.linalg.solve(L, -g))
        t = t + d[:3]
        w = d[3:]
        th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        if th2 < 1e-16:
            E = np.eye(3) + K
        else:
            th = np.sqrt(th2)
            E = (np.eye(3) + (np.sin(th) / th) * K) + ((1 - np.cos(th)) / th2) * (K @ K)
        R = E @ R
        iterations += 1
    return dict(R=R, t=t, H=H, g=g, cost=cost, candidates=len(records), used=used, iterations=iterations, status=status)


# ---- crafted inputs ---------------------------------------------------------------------------------------------------------
def craft_arrays(n, seed, fm, width, height, outliers=0.0, parallel=False):
    """n keyframe keylines and the n current keylines they move to under the crafted motion. Keyframe: pos_img uniform inside the
    frame (principal-point coordinates), rho in [0.2, 2], sigma_rho = 0.05 rho, matches 3. Current: the exact projection rounded to
    fp32, gradients of uniform direction and norm 5..50 (parallel: all along x, so that J[1] == 0 in every term and H is singular
    exactly); outliers: that share of the current keylines displaced by +-15 px along their normal."""
    rng = np.random.default_rng(seed)
    fm = F32(fm)
    pos = np.stack([rng.uniform(-0.45 * width, 0.45 * width, n), rng.uniform(-0.45 * height, 0.45 * height, n)], 1).astype(F32)
    rho = rng.uniform(0.2, 2.0, n).astype(F32)
    prs4 = np.concatenate([pos, rho[:, None], (F32(0.05) * rho).astype(F32)[:, None]], 1).astype(F32)
    R, t = true_motion()
    a = (pos[:, 0] / fm).astype(F32).astype(np.float64)
    b = (pos[:, 1] / fm).astype(F32).astype(np.float64)
    Y = np.stack([a, b, np.ones(n)], 1) @ R.T + rho.astype(np.float64)[:, None] * t
    assert (Y[:, 2] > 0.5).all()
    cur = np.float64(fm) * Y[:, :2] / Y[:, 2:3]
    ang = rng.uniform(0, 2 * np.pi, n)
    norm = rng.uniform(5.0, 50.0, n)
    if parallel:
        ang = np.zeros(n)
    grad = np.stack([norm * np.cos(ang), norm * np.sin(ang)], 1).astype(F32)
    if parallel:
        assert (grad[:, 1] == 0).all()
    n_out = int(round(outliers * n))
    if n_out:
        idx = rng.choice(n, n_out, replace=False)
        unit = grad[idx].astype(np.float64) / np.linalg.norm(grad[idx].astype(np.float64), axis=1)[:, None]
        cur[idx] += 15.0 * rng.choice([-1.0, 1.0], n_out)[:, None] * unit
    return dict(prs4=prs4, kf_matches=np.full(n, 3, np.uint32), cur_pos_img=cur.astype(F32), cur_grad=grad)


def identity_records(n):
    """keyframe keyline j lives on as current keyline j"""
    rec = np.zeros(n, KF_MATCH_DTYPE)
    rec["kf_keyline"] = rec["keyline"] = np.arange(n)
    rec["claimants"] = 1
    return rec


def craft_keylines(base_kf, base_cur, A):
    """The arrays of craft_arrays written into keyline arrays of two maps (the first len(A) keylines of each; a longer current map
    keeps match_id_keyframe = -1 behind them). Returns (keyframe keylines, current keylines)."""
    n = len(A["prs4"])
    assert len(base_kf) >= n and len(base_cur) >= n
    kf, cur = base_kf.copy(), base_cur.copy()
    kf["pos_img"][:n] = A["prs4"][:, :2]
    kf["rho"][:n], kf["sigma_rho"][:n], kf["matches"][:n] = A["prs4"][:, 2], A["prs4"][:, 3], A["kf_matches"]
    cur["match_id_keyframe"] = -1
    cur["match_id_keyframe"][:n] = np.arange(n)
    cur["pos_img"][:n] = A["cur_pos_img"]
    cur["gradient"][:n] = A["cur_grad"]
    cur["sigma_rho"][:n] = F32(0.1)      # (the winner's key; one claimant per slot here)
    return kf, cur


def off_guess(seed=0):
    """a guess 0.03 rad and 10 % of |t| off the crafted motion"""
    rng = np.random.default_rng(100 + seed)
    R, t = true_motion()
    w = rng.normal(size=3)
    d = rng.normal(size=3)
    return rodrigues(0.03 * w / np.linalg.norm(w)) @ R, t + 0.1 * np.linalg.norm(t) * d / np.linalg.norm(d)
