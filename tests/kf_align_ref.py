"""The alignment of a keyframe snapshot through a map's distance field (rebvio_hip_map_keyframe_align) restated in numpy float64,
expression by expression after the comment in include/rebvio_hip.h, and the crafted inputs the alignment tests share. A plain helper
module like support.py and kf_pose_ref.py: no test lives here and importing it needs no GPU."""
import numpy as np

from kf_pose_ref import DEFAULT_FILTER, N_SUMS, _terms, pose_sums, true_motion, unpack_sums
from support import F32, KF_MATCH_DTYPE, rodrigues

GUARD = 1e-9      # no term may come this close to a cell edge (px), to the gate or to the Huber switch where two sides are compared
OFFSETS = ((0.005, 0.02), (0.02, 0.08))      # (rad along (1, -1, 1), units along (-1, 1, 1)) off the crafted motion
# |device - numpy| over R and t of the solves of test_solve_from_the_offsets (tests/test_keyframe_align_gpu.py) - measured maximum on
# an MI355X: 2.22e-16 (device sin / cos and the Cholesky order differ from numpy's by a few ulp, amplified by cond(H) of 17); the
# bound is 100 x that. It has to stay <= 0.1 x the restatement's own error from the crafted motion (1.09e-9 at the least), which the
# test asserts as a condition. (The displaced-keyline solves and the re-acquisition, held to the same bound, measured 2.22e-16 and
# 1.8e-16 at most; the rows of tests/context_cases.py, cond(H) 17 to 71, 2.22e-16 at most.)
DEV_VS_NP = 2.22e-14
LOOKUP_EXITS = ("Y.z", "border", "empty cell", "max_dist", "min_cos", "zero gradient")      # where a keyline can leave steps 2..6


def unit_of(kl):
    """gradient / gradient_norm of downloaded keylines as DistanceField::build forms it (fp32 IEEE divisions); zeros where the norm
    is not > 0 (rebvio_hip_kf_snapshot_add_normals' rule)"""
    g = np.asarray(kl["gradient"], F32).reshape(-1, 2)
    gn = np.asarray(kl["gradient_norm"], F32).reshape(-1)
    with np.errstate(all="ignore"):
        u = (g / gn[:, None]).astype(F32)
    u[~(gn > 0)] = 0
    return u


def offset_guess(rot, trans, sign=1.0):
    """the crafted motion displaced by rot * (1, -1, 1) rad (applied on the left) and trans * (-1, 1, 1) units"""
    R, t = true_motion()
    return rodrigues(sign * rot * np.array([1.0, -1.0, 1.0])) @ R, t + sign * trans * np.array([-1.0, 1.0, 1.0])


def _lookup(cam, prs4, normals, cur_pos, cur_unit, ids, dists, R, t, min_cos, max_dist):
    """steps 2..5 of the definition for every keyframe keyline: (ok mask, owner i (0 where not ok), guards); guards["why"] = the step
    a keyline left at (LOOKUP_EXITS' order, 1-based; 0 where ok)"""
    fm, cx, cy, rows, cols = cam
    fm, cx, cy = F32(fm), F32(cx), F32(cy)
    R = np.asarray(R, np.float64).reshape(9)
    t = np.asarray(t, np.float64).reshape(3)
    k = np.asarray(prs4, F32).reshape(-1, 4)
    n = len(k)
    ids = np.asarray(ids, np.int64).reshape(-1)
    dists = np.asarray(dists, np.int64).reshape(-1)
    pos = np.asarray(cur_pos, F32).reshape(-1, 2)
    unit = np.asarray(cur_unit, F32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        a = (k[:, 0] / fm).astype(F32).astype(np.float64)
        b = (k[:, 1] / fm).astype(F32).astype(np.float64)
        rho = k[:, 2].astype(np.float64)
        Z = [(R[3 * r] * a + R[3 * r + 1] * b) + R[3 * r + 2] for r in range(3)]
        Y = [Z[r] + rho * t[r] for r in range(3)]
        ok = Y[2] > 0
        why = np.where(ok, 0, 1)
        px, py = Y[0] / Y[2], Y[1] / Y[2]
        u = np.float64(fm) * px + np.float64(cx)
        v = np.float64(fm) * py + np.float64(cy)
        uh, vh = u + 0.5, v + 0.5
        x, y = np.floor(uh), np.floor(vh)
        projected = ok.copy()
        ok &= (x >= 1) & (x <= cols - 2) & (y >= 1) & (y <= rows - 2)
        why[(why == 0) & ~ok] = 2
        cell = np.where(ok, y * cols + x, 0).astype(np.int64)
        i = ids[cell] if len(ids) else np.zeros(n, np.int64)
        d = dists[cell] if len(ids) else np.zeros(n, np.int64)
        ok &= i >= 0
        why[(why == 0) & ~ok] = 3
        ok &= d <= max_dist
        why[(why == 0) & ~ok] = 4
        i = np.where(ok, i, 0)
        ni = unit[i].astype(np.float64) if len(unit) else np.zeros((n, 2))
        gate_d = np.full(n, np.inf)
        if normals is not None and min_cos > -1.0:
            nj = np.asarray(normals, F32).reshape(-1, 2).astype(np.float64)
            mx = R[0] * nj[:, 0] + R[1] * nj[:, 1]
            my = R[3] * nj[:, 0] + R[4] * nj[:, 1]
            mm = mx * mx + my * my
            nn = ni[:, 0] * ni[:, 0] + ni[:, 1] * ni[:, 1]
            dot = mx * ni[:, 0] + my * ni[:, 1]
            bound = (min_cos * np.sqrt(mm)) * np.sqrt(nn)
            gated = ok & (mm > 0) & (nn > 0)
            gate_d[gated] = np.abs(dot - bound)[gated]
            ok &= ~gated | (dot >= bound)
            why[(why == 0) & ~ok] = 5
        # distance of u + 0.5 / v + 0.5 from the nearest integer: how close the projection is to a cell edge (all projected terms)
        edge = np.minimum(np.abs(uh - np.rint(uh)), np.abs(vh - np.rint(vh)))
        edge = np.where(projected & np.isfinite(edge), edge, np.inf)
    return ok, i, dict(edge=edge, gate=gate_d, why=why)


def _residual(fm, prs4, q, unit, i, R, t):
    """e of the definition for (j, i[j]) - the arithmetic of kf_pose_ref._terms up to e"""
    fm = F32(fm)
    R = np.asarray(R, np.float64).reshape(9)
    t = np.asarray(t, np.float64).reshape(3)
    k = np.asarray(prs4, F32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        a = (k[:, 0] / fm).astype(F32).astype(np.float64)
        b = (k[:, 1] / fm).astype(F32).astype(np.float64)
        rho = k[:, 2].astype(np.float64)
        qq = q[i]
        qx = (qq[:, 0] / fm).astype(F32).astype(np.float64)
        qy = (qq[:, 1] / fm).astype(F32).astype(np.float64)
        g = unit[i].astype(np.float64)
        gn = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1])
        nx, ny = g[:, 0] / gn, g[:, 1] / gn
        Z = [(R[3 * r] * a + R[3 * r + 1] * b) + R[3 * r + 2] for r in range(3)]
        Y = [Z[r] + rho * t[r] for r in range(3)]
        return np.float64(fm) * (nx * (Y[0] / Y[2] - qx) + ny * (Y[1] / Y[2] - qy))


def np_kf_align_sums(cam, prs4, kf_matches, normals, cur_pos, cur_unit, ids, dists, R, t, flt=DEFAULT_FILTER, huber=2.0, min_cos=0.9,
                     max_dist=40):
    """One evaluation at (R, t): (sums [28], sum of |term| per sum [28], used, assoc int32 [n] (-1: not used), guards) - guards: the
    smallest distance of any term from a cell edge (px), from the gate's switch and of |e| from huber"""
    fm, cx, cy, rows, cols = cam
    prs4 = np.asarray(prs4, F32).reshape(-1, 4)
    n = len(prs4)
    pos = np.asarray(cur_pos, F32).reshape(-1, 2)
    unit = np.asarray(cur_unit, F32).reshape(-1, 2)
    ok, i, guards = _lookup(cam, prs4, normals, pos, unit, ids, dists, R, t, min_cos, max_dist)
    q = (pos - np.array([F32(cx), F32(cy)], F32)).astype(F32)       # pos - (cx, cy): fp32 subtractions
    rec = np.zeros(n, KF_MATCH_DTYPE)
    rec["kf_keyline"], rec["keyline"] = np.arange(n), i
    if n and len(pos):
        ok_t, terms = _terms(fm, prs4, kf_matches, q, unit, rec, R, t, flt, huber)
        e = _residual(fm, prs4, q, unit, i, R, t)
    else:
        ok_t, terms, e = np.zeros(n, bool), np.zeros((n, N_SUMS)), np.zeros(n)
    used = ok & ok_t
    terms[~used] = 0.0
    with np.errstate(all="ignore"):
        hub = np.abs(np.abs(e) - huber)
    g = dict(edge=float(guards["edge"].min()) if n else np.inf, gate=float(guards["gate"].min()) if n else np.inf,
             huber=float(hub[used].min()) if used.any() else np.inf)
    assoc = np.where(used, i, -1).astype(np.int32)
    return terms.sum(0), np.abs(terms).sum(0), int(used.sum()), assoc, g


def np_kf_align(cam, prs4, kf_matches, normals, cur_pos, cur_unit, ids, dists, R0=None, t0=None, flt=DEFAULT_FILTER, huber=2.0,
                min_cos=0.9, max_dist=40, max_iter=8, min_used=12):
    """The whole solve: max_iter + 1 evaluations, a Cholesky step behind every one but the last (the loop of kf_pose_ref.np_kf_pose).
    A dict with the fields of rebvio_hip_kf_pose, assoc of the last evaluation, and guard = the smallest guard distance over all
    evaluations."""
    R = np.eye(3) if R0 is None else np.array(R0, np.float64).reshape(3, 3)
    t = np.zeros(3) if t0 is None else np.array(t0, np.float64).reshape(3)
    n = len(np.asarray(prs4).reshape(-1, 4))
    status = iterations = 0
    guard = np.inf
    H, g, cost, used, assoc = np.zeros((6, 6)), np.zeros(6), 0.0, 0, np.zeros(0, np.int32)
    if n == 0:
        status = 3
    for it in range(max_iter + 1 if n else 0):
        S, _, used, assoc, gd = np_kf_align_sums(cam, prs4, kf_matches, normals, cur_pos, cur_unit, ids, dists, R, t, flt, huber, min_cos,
                                                 max_dist)
        guard = min(guard, gd["edge"], gd["gate"], gd["huber"])
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
    return dict(R=R, t=t, H=H, g=g, cost=cost, candidates=n, used=used, iterations=iterations, status=status, assoc=assoc, guard=guard)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
_SCENES = {}


def oracle_scene(O, frame=2, width=160, height=120, seed=1, **kw):
    """Frame `frame` of the synthetic stream detected by the oracle (after the frames before it, so the threshold servo has run), its
    distance field, and the keyframe keylines crafted against it. **kw: parameters of the oracle's context; fm, cx and cy among them
    replace the synthetic camera's in `cam` as well. Computed once per argument set; treat it as read-only.
    dict(cam, search_range, kl, pos, unit, ids, dists, craft)"""
    key = (frame, width, height, seed, tuple(sorted(kw.items())))
    if key not in _SCENES:
        from conftest import params_for
        from rebvio_amd import synth
        frames, cam = synth.render_stream(width, height, frame + 1)
        orc = O.Oracle(params_for(O, cam, **kw))
        for k in range(frame + 1):
            m = orc.detect_u8(frames[k], k * 50000)
        orc.build_distance_field(m)
        ids, dists = orc.distance_field()
        kl = m.keylines()
        camt = (kw.get("fm", cam.fm), kw.get("cx", cam.cx), kw.get("cy", cam.cy), height, width)      # the camera the oracle was given
        _SCENES[key] = dict(cam=camt, search_range=int(orc.p.search_range), kl=kl, pos=np.ascontiguousarray(kl["pos"]), unit=unit_of(kl),
                            ids=ids.reshape(-1), dists=dists.reshape(-1), craft=craft_against(kl, ids, dists, seed, camt))
    return _SCENES[key]


# ---- crafted inputs ---------------------------------------------------------------------------------------------------------
def craft_against(kl, ids, dists, seed, cam, displaced=0.0):
    """Keyframe keylines behind the crafted motion (kf_pose_ref.true_motion) for a detected map: one per keyline i of `kl` that owns
    its own cell (the cell its pos rounds to, inside tryVel's bounds) at distance 0. The point of keyline i at depth 1 / rho, rho
    uniform in [0.2, 2], is X_cur; X_kf = R^T (X_cur - t) gives pos_img and rho of the keyframe keyline, rounded to fp32; its
    normal is R^T n_i (the image block), renormalised; sigma_rho = 0.05 rho, matches 3. displaced: that share of the keyframe
    keylines moved by 15 px along their normal. Returns dict(prs4, kf_matches, normals, owner)."""
    fm, cx, cy, rows, cols = cam
    rng = np.random.default_rng(seed)
    ids = np.asarray(ids).reshape(rows, cols)
    dists = np.asarray(dists).reshape(rows, cols)
    pos = np.asarray(kl["pos"], F32).reshape(-1, 2).astype(np.float64)
    x, y = np.floor(pos[:, 0] + 0.5).astype(np.int64), np.floor(pos[:, 1] + 0.5).astype(np.int64)
    inside = (x >= 1) & (x <= cols - 2) & (y >= 1) & (y <= rows - 2)
    xc, yc = np.clip(x, 0, cols - 1), np.clip(y, 0, rows - 1)
    unit = unit_of(kl).astype(np.float64)
    own = inside & (ids[yc, xc] == np.arange(len(pos))) & (dists[yc, xc] == 0) & ((unit ** 2).sum(1) > 0)
    owner = np.flatnonzero(own)
    n = len(owner)
    R, t = true_motion()
    rho_cur = rng.uniform(0.2, 2.0, n)
    ray = np.stack([(pos[owner, 0] - np.float64(F32(cx))) / np.float64(F32(fm)), (pos[owner, 1] - np.float64(F32(cy))) / np.float64(F32(fm)),
                    np.ones(n)], 1)
    X_kf = (ray / rho_cur[:, None] - t) @ R          # rows: R^T (X_cur - t)
    assert (X_kf[:, 2] > 0.2).all()
    kf_pos = np.float64(F32(fm)) * X_kf[:, :2] / X_kf[:, 2:3]
    nrm = unit[owner] @ R[:2, :2]                    # rows: R[:2, :2]^T n_i
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    n_out = int(round(displaced * n))
    if n_out:
        idx = rng.choice(n, n_out, replace=False)
        kf_pos[idx] += 15.0 * rng.choice([-1.0, 1.0], n_out)[:, None] * nrm[idx]
    rho = (1.0 / X_kf[:, 2]).astype(F32)
    prs4 = np.concatenate([kf_pos.astype(F32), rho[:, None], (F32(0.05) * rho).astype(F32)[:, None]], 1).astype(F32)
    return dict(prs4=prs4, kf_matches=np.full(n, 3, np.uint32), normals=nrm.astype(F32), owner=owner.astype(np.int32))


def craft_kf_keylines(base, A, n=None):
    """the first n (default: all) crafted keyframe keylines written into the first n keylines of `base` (a keyline array of at least
    that size): pos_img, rho, sigma_rho, matches, and gradient = 10 x the normal with gradient_norm 10"""
    n = len(A["prs4"]) if n is None else n
    assert len(base) >= n and len(A["prs4"]) >= n
    kf = base.copy()
    kf["pos_img"][:n] = A["prs4"][:n, :2]
    kf["rho"][:n], kf["sigma_rho"][:n], kf["matches"][:n] = A["prs4"][:n, 2], A["prs4"][:n, 3], A["kf_matches"][:n]
    kf["gradient"][:n] = (F32(10.0) * A["normals"][:n]).astype(F32)
    kf["gradient_norm"][:n] = F32(10.0)
    return kf


def lookup_case(cam, pos, unit, ids, dists, A, room, zero_gradient):
    """The keyframe keylines of `A` (craft_against) with one planted keyline per exit of LOOKUP_EXITS behind them, `room` keylines
    at the most, for the crafted motion and the default filter. The plants are made like the crafted keylines: the point of a
    current pixel, 0.2 px off its cell's centre, at depth 1, taken back through the crafted motion.
      Y.z            pos_img = (-30 fm, 0): Z.z = R[2, 0] (-30) + R[2, 2] < 0, and rho 0.5 adds only 0.05
      border         a pixel of column 0
      empty cell     the first cell inside the border that no keyline reaches
      max_dist       the cell inside the border farthest from its owner, at max_dist = that distance less one
      min_cos        the cell of a keyline that owns it, with the normal turned by a quarter
      zero gradient  no plant: the unit of one crafted keyline's owner is set to zero in the returned copy of `unit`. Only where the
                     caller hands the arrays over itself (zero_gradient): a detected map has no such keyline.
    Returns dict(prs4, kf_matches, normals, pos, unit, ids, dists, max_dist, plants {exit: keyframe keyline})."""
    fm, cx, cy, rows, cols = cam
    R, t = true_motion()
    ids2, dists2 = np.asarray(ids).reshape(rows, cols), np.asarray(dists).reshape(rows, cols)
    pos, unit = np.asarray(pos, F32).reshape(-1, 2), np.array(unit, F32).reshape(-1, 2)
    inner = np.zeros((rows, cols), bool)
    inner[1:rows - 1, 1:cols - 1] = True
    ey, ex = np.argwhere((ids2 < 0) & inner)[0]
    far = np.where((ids2 >= 0) & inner, dists2, -1)
    fy, fx = np.unravel_index(far.argmax(), far.shape)
    max_dist = int(dists2[fy, fx]) - 1
    assert max_dist >= 1
    own = A["owner"]
    centred = [k for k, i in enumerate(own) if np.abs(pos[i] - np.round(pos[i])).max() < 0.3]
    k_cos, k_zero = centred[0], centred[1]
    gx, gy = np.round(pos[own[k_cos]]).astype(int)
    un = unit[own[k_cos]].astype(np.float64)

    def onto(x, y, normal):
        ray = np.array([(x + 0.2 - np.float64(F32(cx))) / np.float64(F32(fm)), (y - 0.2 - np.float64(F32(cy))) / np.float64(F32(fm)), 1.0])
        X = R.T @ (ray - t)
        n = R[:2, :2].T @ np.asarray(normal, np.float64)
        return [fm * X[0] / X[2], fm * X[1] / X[2], 1.0 / X[2], 0.05 / X[2]], n / np.linalg.norm(n)

    made = {"Y.z": ([-30.0 * fm, 0.0, 0.5, 0.025], un), "border": onto(0, rows // 2, un), "empty cell": onto(ex, ey, un),
            "max_dist": onto(fx, fy, unit[ids2[fy, fx]].astype(np.float64)), "min_cos": onto(gx, gy, (-un[1], un[0]))}
    n = min(len(A["prs4"]), room - len(made))
    assert n > k_zero
    plants = {name: n + k for k, name in enumerate(made)}
    if zero_gradient:
        unit[own[k_zero]] = 0
        plants["zero gradient"] = k_zero
    return dict(prs4=np.concatenate([A["prs4"][:n], np.array([m[0] for m in made.values()], F32)]).astype(F32),
                kf_matches=np.full(n + len(made), 3, np.uint32),
                normals=np.concatenate([A["normals"][:n], np.array([m[1] for m in made.values()], F32)]).astype(F32),
                pos=pos, unit=unit, ids=np.asarray(ids).reshape(-1), dists=np.asarray(dists).reshape(-1), max_dist=max_dist, plants=plants)


def assert_lookup_case_is_not_vacuous(cam, prs4, normals, pos, unit, ids, dists, max_dist, plants, flt_ok):
    """On the restatement, at the crafted motion and min_cos 0.9: every planted keyline leaves the lookup at its own exit and at least
    half of all keyframe keylines (flt_ok: those that pass the filter) come through with an owner whose gradient has a direction.
    Returns that mask."""
    R, t = true_motion()
    ok, i, g = _lookup(cam, prs4, normals, pos, unit, ids, dists, R, t, 0.9, max_dist)
    zero = ok & ~((np.asarray(unit, F32).reshape(-1, 2)[i].astype(np.float64) ** 2).sum(1) > 0)
    why = np.where(zero, 6, g["why"])
    for name, j in plants.items():
        assert flt_ok[j] and why[j] == 1 + LOOKUP_EXITS.index(name), (name, j, int(why[j]))
    assoc = ok & ~zero & flt_ok
    assert 2 * int(assoc.sum()) >= len(prs4), (int(assoc.sum()), len(prs4))
    return assoc


# ---- what the device tests share (B = the backend module) ---------------------------------------------------------------------------
def cam_of(ctx):
    return (ctx.p.fm, ctx.p.cx, ctx.p.cy, ctx.rows, ctx.cols)


def current_data(mc):
    """what the restatement is given of the current map: pos, unit, the field - downloaded"""
    kl = mc.keylines()
    ids, dists = mc.distance_field()
    return kl, (np.ascontiguousarray(kl["pos"]), unit_of(kl), ids.reshape(-1), dists.reshape(-1))


def data_of(ctx, snap, cur, normals=True):
    prs4, mt = snap.download()
    return (cam_of(ctx), prs4, mt, snap.normals() if normals else None, *cur)


def same_bytes(a, b):
    return bytes(a) == bytes(b)


def np_kw(opts):
    return {("huber" if k == "huber_px" else k): v for k, v in opts.items()}


def assert_evaluation(B, ctx, mc, snap, D, R, t, what, **opts):
    """one evaluation (max_iter 0) at (R, t): the restatement's guards, assoc element for element, the 28 sums within the bound, the
    pose untouched, a second call equal in every byte"""
    S, absS, used, assoc, g = np_kf_align_sums(*D, R, t, **np_kw(opts))
    assert min(g.values()) > GUARD, (what, g)
    o = B.default_kf_align_opts(ctx, max_iter=0, **opts)
    got, a = mc.keyframe_align(snap, o, R, t, want_assoc=True)
    assert np.array_equal(a, assoc), (what, np.flatnonzero(a != assoc)[:8], a[a != assoc][:8], assoc[a != assoc][:8])
    assert got.used == used and got.candidates == len(D[1]) and got.iterations == 0, (what, got.used, used, got.candidates)
    assert got.status == (3 if used < 12 else 0)
    assert np.array_equal(np.array(got.R), np.asarray(R, np.float64).reshape(9)) and np.array_equal(np.array(got.t), np.asarray(t, np.float64))
    d = np.abs(pose_sums(got) - S)
    bound = (used + 64) * 2.0 ** -52 * absS
    assert (d <= bound).all(), (what, np.flatnonzero(d > bound), d[d > bound], bound[d > bound])
    again, a2 = mc.keyframe_align(snap, o, R, t, want_assoc=True)
    assert same_bytes(got, again) and np.array_equal(a, a2), what
    return used
