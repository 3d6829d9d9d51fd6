"""The numpy / Python-float restatement of the straight segments (include/rebvio_hip.h is the definition), written from the header: the
splits as plain level-synchronous loops over lists of segments, the fit's sums in the stated 16-partial order with Python floats
(IEEE doubles: one rounding per operation). The hook and the device are compared with it by equality of record bytes and counts.
Also the planted maps more than one test file uses."""
import math

import numpy as np

from edge_chains_ref import DEFAULT_FILTER, links_of_sequences, np_polylines
from support import F32

LINE_SEGMENT_DTYPE = np.dtype([("xyz0", "<f4", (3,)), ("xyz1", "<f4", (3,)), ("uv0", "<f4", (2,)), ("uv1", "<f4", (2,)), ("rho0", "<f4"),
                               ("rho1", "<f4"), ("sigma_rho0", "<f4"), ("sigma_rho1", "<f4"), ("max_dev2", "<f4"), ("chi2", "<f4"),
                               ("first_point", "<i4"), ("points", "<i4"), ("line", "<i4"), ("flags", "<i4")])
COUNT_FIELDS = ("segments_all", "kept", "depth_valid", "unresolved", "rounds_used", "points", "lines", "reserved")
ENTRIES = ("rebvio_hip_default_segment_opts", "rebvio_hip_map_edge_segments", "rebvio_hip_test_edge_segments_host")
KERNELS_SEG = ("k_seg_init", "k_seg_far", "k_seg_split", "k_seg_count", "k_seg_emit", "k_seg_fit")
IDENTITY = (np.eye(3, dtype=F32), np.zeros(3, F32), F32(1.0))


def seg_launches(max_rounds):
    """the segment launches behind the polylines' R + 8"""
    return 2 * max_rounds + 5


def bits(x):
    return int(np.array(x, F32).view(np.uint32))


def dev2(qa, qb, qp):
    """the squared deviation of the definition, one fp32 rounding per operation"""
    ex, ey, px, py = F32(qb[0] - qa[0]), F32(qb[1] - qa[1]), F32(qp[0] - qa[0]), F32(qp[1] - qa[1])
    l2 = F32(F32(ex * ex) + F32(ey * ey))
    cr = F32(F32(ex * py) - F32(ey * px))
    d2 = F32(F32(px * px) + F32(py * py)) if l2 == 0 else F32(F32(cr * cr) / l2)
    return d2 if d2 >= 0 else F32(0)


def winner(q, a, b):
    """(d2, m) of segment [a, b]: the largest key; (0, None) without an interior point"""
    best = None
    for p in range(a + 1, b):
        d2 = dev2(q[a], q[b], q[p])
        key = (bits(d2) << 32) | (0xFFFFFFFF - p)
        if best is None or key > best[0]:
            best = (key, d2, p)
    return (F32(0), None) if best is None else (best[1], best[2])


def xyz_of(fm, pose, px, py, rho):
    R, t, scale = pose
    R, t = np.asarray(R, F32).reshape(9), np.asarray(t, F32).reshape(3)
    with np.errstate(all="ignore"):
        u, v = F32(F32(px) / F32(fm)), F32(F32(py) / F32(fm))
        z = F32(F32(scale) / F32(rho))
        xc, yc = F32(u * z), F32(v * z)
        return [F32(F32(F32(F32(R[3 * i] * xc) + F32(R[3 * i + 1] * yc)) + F32(R[3 * i + 2] * z)) + t[i]) for i in range(3)]


def fit(q, rho, sig, a, b):
    """(r0, r1, v0, v1, chi2, det) in Python floats, the sums in the 16-partial pairwise order"""
    with np.errstate(all="ignore"):
        ex, ey = F32(q[b][0] - q[a][0]), F32(q[b][1] - q[a][1])
        l2 = F32(F32(ex * ex) + F32(ey * ey))
        part = [[0.0] * 6 for _ in range(16)]
        for i in range(b - a + 1):
            p = a + i
            px, py = F32(q[p][0] - q[a][0]), F32(q[p][1] - q[a][1])
            t = float(F32(F32(F32(px * ex) + F32(py * ey)) / l2))
            sg = F32(abs(F32(sig[p])))
            if not sg >= F32(1e-6):
                sg = F32(1e-6)
            w = 1.0 / (float(sg) * float(sg))
            r = float(F32(rho[p]))
            wt, wr = w * t, w * r
            s = part[i % 16]
            for k, term in enumerate((w, wt, wt * t, wr, wt * r, wr * r)):
                s[k] = s[k] + term
    width = 1
    while width < 16:
        for j in range(0, 16, 2 * width):
            part[j] = [x + y for x, y in zip(part[j], part[j + width])]
        width *= 2
    Sw, Swt, Swtt, Swr, Swtr, Swrr = part[0]

    def div(x, y):
        with np.errstate(all="ignore"):
            return float(np.float64(x) / np.float64(y))
    det = Sw * Swtt - Swt * Swt
    r0 = div(Swtt * Swr - Swt * Swtr, det)
    sl = div(Sw * Swtr - Swt * Swr, det)
    r1 = r0 + sl
    v0 = div(Swtt, det)
    v1 = div((Swtt - 2 * Swt) + Sw, det)
    chi2 = Swrr - (r0 * Swr + sl * Swtr)
    if not chi2 > 0:
        chi2 = 0.0
    return r0, r1, v0, v1, chi2, det


def np_segments(kl, fm, flt=DEFAULT_FILTER, min_chain_length=8, pose=None, tol=1.0, min_length=4.0, min_points=8, max_rounds=16):
    """(segments LINE_SEGMENT_DTYPE, counts dict) of a KEYLINE_DTYPE array"""
    with np.errstate(all="ignore"):
        return _np_segments(kl, fm, flt, min_chain_length, pose, tol, min_length, min_points, max_rounds)


def _np_segments(kl, fm, flt, min_chain_length, pose, tol, min_length, min_points, max_rounds):
    pose = IDENTITY if pose is None else pose
    pts, _, lines = np_polylines(kl, fm, flt, min_chain_length, pose)
    key = pts["keyline"]
    q = [(F32(kl["pos_img"][k][0]), F32(kl["pos_img"][k][1])) for k in key]
    rho, sig = [kl["rho"][k] for k in key], [kl["sigma_rho"][k] for k in key]
    tol2 = F32(F32(tol) * F32(tol))
    min_len2 = F32(F32(min_length) * F32(min_length))
    segs = []                                     # (a, b, line) in point order
    for l, ln in enumerate(lines):
        first, n = int(ln["first_point"]), int(ln["points"])
        if n >= 2:
            segs.append((first, first + n - 1, l))
    rounds_used = 0
    for _ in range(max_rounds):                   # level-synchronous: every segment of the round's start is tested once
        nxt, split = [], False
        for a, b, l in segs:
            d2, m = winner(q, a, b)
            if m is not None and d2 > tol2:
                nxt += [(a, m, l), (m, b, l)]
                split = True
            else:
                nxt.append((a, b, l))
        segs = nxt
        if not split:
            break
        rounds_used += 1
    out, unresolved, valid = [], 0, 0
    for a, b, l in segs:
        d2, _ = winner(q, a, b)
        unres = bool(d2 > tol2)
        unresolved += unres
        with np.errstate(all="ignore"):
            ex, ey = F32(q[b][0] - q[a][0]), F32(q[b][1] - q[a][1])
            l2 = F32(F32(ex * ex) + F32(ey * ey))
        if not (b - a + 1 >= min_points and l2 >= min_len2):
            continue
        r0, r1, v0, v1, chi2, det = fit(q, rho, sig, a, b)
        rec = np.zeros((), LINE_SEGMENT_DTYPE)
        with np.errstate(all="ignore"):
            f0, f1 = F32(r0), F32(r1)
        ok = bool(det > 0 and v0 >= 0 and v1 >= 0 and F32(flt[2]) <= f0 <= F32(flt[3]) and F32(flt[2]) <= f1 <= F32(flt[3]))
        if ok:
            rec["xyz0"], rec["xyz1"] = xyz_of(fm, pose, q[a][0], q[a][1], f0), xyz_of(fm, pose, q[b][0], q[b][1], f1)
            rec["rho0"], rec["rho1"] = f0, f1
            rec["sigma_rho0"], rec["sigma_rho1"] = F32(math.sqrt(v0)), F32(math.sqrt(v1))
        rec["uv0"], rec["uv1"] = q[a], q[b]
        rec["max_dev2"] = d2
        with np.errstate(all="ignore"):
            rec["chi2"] = F32(chi2)
        rec["first_point"], rec["points"], rec["line"], rec["flags"] = a, b - a + 1, l, int(ok) | (2 if unres else 0)
        valid += ok
        out.append(rec)
    counts = dict(segments_all=len(segs), kept=len(out), depth_valid=valid, unresolved=unresolved, rounds_used=rounds_used, points=len(pts),
                  lines=len(lines), reserved=0)
    return (np.array(out, LINE_SEGMENT_DTYPE) if out else np.zeros(0, LINE_SEGMENT_DTYPE)), counts


def assert_segments_equal(got, want, what="", cap=None):
    """got = (segments, SegmentCounts) of the entry or the hook; want = np_segments() or another got"""
    segs, counts = got
    wsegs, wcounts = want
    counts = counts if isinstance(counts, dict) else counts.as_dict()
    wcounts = wcounts if isinstance(wcounts, dict) else wcounts.as_dict()
    assert counts == wcounts, (what, counts, wcounts)
    wsegs = wsegs if cap is None else wsegs[:cap]
    assert len(segs) == len(wsegs), (what, len(segs), len(wsegs))
    if segs.tobytes() != wsegs.tobytes():
        bad = [i for i in range(len(segs)) if segs[i].tobytes() != wsegs[i].tobytes()]
        raise AssertionError((what, "records differ", bad[:8], segs[bad[0]], wsegs[bad[0]]))


# ---- planted maps: keylines in index order along one or more paths ------------------------------------------------------------
def keylines_on_paths(dtype, paths_xy, rho=1.0, sigma=0.05, extra=0):
    """KEYLINE_DTYPE of the points of every path (a list of (x, y) lists), linked in order; `extra` unlinked keylines behind them.
    Everything passes the default filter (matches 3)."""
    n = sum(len(p) for p in paths_xy) + extra
    seqs, at = [], 0
    for p in paths_xy:
        seqs.append(list(range(at, at + len(p))))
        at += len(p)
    idp, idn = links_of_sequences(n, paths=[s for s in seqs if len(s) > 1])
    kl = np.zeros(n, dtype)
    xy = np.array([pt for p in paths_xy for pt in p], F32).reshape(-1, 2)
    kl["pos_img"][:len(xy)] = xy
    kl["pos"] = kl["pos_img"] + F32(80)
    kl["rho"] = F32(rho)
    kl["sigma_rho"] = F32(sigma)
    kl["gradient_norm"] = F32(3)
    kl["matches"] = 3
    kl["id"] = np.arange(n)
    kl["id_prev"], kl["id_next"] = idp, idn
    kl["match_id"] = kl["match_id_forward"] = kl["match_id_keyframe"] = -1
    return kl


def straight(n, x0=-50.0, y0=-20.0, dx=1.0, dy=0.5):
    return [(x0 + dx * i, y0 + dy * i) for i in range(n)]


def zigzag(n, amp=3.0):
    return [(float(i) * 0.001 if n > 4096 else float(i), amp * (i % 2)) for i in range(n)]


def arc_chain(depth, radius=400.0, angle=math.pi / 2):
    """2^depth + 1 points on a circle arc: every level of the bisection finds its farthest point in the middle, so it takes exactly
    `depth` rounds while the sagitta of two steps (radius * (1 - cos(angle / 2^depth)), 1.9 px at depth 4) is above the tolerance"""
    n = (1 << depth) + 1
    ang = np.linspace(0.0, angle, n)
    return [(float(radius * math.cos(a)), float(radius * math.sin(a))) for a in ang]


def with_depths(kl):
    """distinct depths along the map: rho in 0.8..1.2 by a fixed pattern, sigma_rho = 0.05 rho"""
    i = np.arange(len(kl))
    kl["rho"] = (F32(0.8) + F32(0.4) * ((i * 7) % 11).astype(F32) / F32(11)).astype(F32)
    kl["sigma_rho"] = (F32(0.05) * kl["rho"]).astype(F32)
    return kl


LOOSE = dict(min_chain_length=2, min_points=2, min_length=0.0)      # every segment of every line of two or more points is kept


def planted_cases(dtype):
    """[(name, keylines, options of np_segments, cap)]: the cases tests/test_edge_segments.py states the answers of by hand"""
    mk = lambda paths: with_depths(keylines_on_paths(dtype, paths))
    cases = [(f"straight {n}", mk([straight(n)]), dict(LOOSE), None) for n in (2, 7, 8, 15, 16, 17, 33)]
    cases.append(("L", mk([[(float(i), 0.0) for i in range(10)] + [(9.0, float(j)) for j in range(1, 10)]]), dict(LOOSE), None))
    # a flat-topped V: points 1 and 2 both lie 2 px from the chord 0 > 3 (d2 = 64 / 16 = 4 exactly); behind the split at 1 point 2
    # lies 16 / 13 = 1.23 px^2 from the chord 1 > 3, below a tolerance of 1.2 px: the tie decides the result
    cases.append(("V tie", mk([[(0.0, 0.0), (1.0, 2.0), (3.0, 2.0), (4.0, 0.0)]]), dict(LOOSE, tol=1.2), None))
    cases.append(("zig-zag", mk([[(float(i), 3.0 * (i % 2)) for i in range(9)]]), dict(LOOSE), None))
    cases.append(("coincident ends", mk([[(0.0, 0.0), (3.0, 0.0), (3.0, 3.0), (0.0, 3.0), (0.0, 0.0)]]), dict(LOOSE), None))
    kl = mk([straight(20)])
    kl["pos_img"][7, 0] = np.nan
    cases.append(("NaN inside", kl, dict(LOOSE), None))
    kl = mk([straight(20)])
    kl["pos_img"][12, 1] = np.inf
    cases.append(("inf inside", kl, dict(LOOSE), None))
    kl = mk([straight(16)])
    kl["sigma_rho"][3], kl["sigma_rho"][8], kl["sigma_rho"][12] = 0.0, -0.02, 1e-9
    cases.append(("sigma 0, negative, tiny", kl, dict(LOOSE), None))
    kl = mk([straight(8)])                                            # seven keylines at rho_min's edge and one far above:
    kl["rho"], kl["sigma_rho"] = F32(0.0011), F32(0.0005)             # the line through them leaves the clamp at the other end
    kl["rho"][7] = 19.0
    cases.append(("fit leaves the clamp", kl, dict(LOOSE), None))
    cases.append(("exactly max_rounds", mk([arc_chain(4)]), dict(LOOSE, max_rounds=4), None))
    cases.append(("one round short", mk([arc_chain(4)]), dict(LOOSE, max_rounds=3), None))
    flat = [(float(i), 0.0) for i in range(8)]                        # 8 points, 7 px long
    cases.append(("min_points met", mk([flat]), dict(min_points=8, min_length=0.0), None))
    cases.append(("min_points missed", mk([flat + [(8.0, 0.0)]]), dict(min_points=10, min_length=0.0, min_chain_length=2), None))
    cases.append(("min_length met", mk([flat]), dict(min_points=2, min_length=7.0), None))
    cases.append(("min_length missed", mk([flat]), dict(min_points=2, min_length=7.001), None))
    cases.append(("cap cut", mk([arc_chain(4), straight(9)]), dict(LOOSE), 3))
    cases.append(("empty", np.zeros(0, dtype), {}, None))
    return cases


def opts_of(B, kw):
    """the SegmentOpts of np_segments' keyword arguments"""
    kw = dict(kw)
    poly = dict(min_chain_length=kw.pop("min_chain_length", 8))
    if "flt" in kw:
        poly["filter"] = dict(zip(("min_matches", "max_rel_sigma", "rho_min", "rho_max"), kw.pop("flt")))
    kw.pop("pose", None)
    return B.default_segment_opts(poly=poly, **kw)


def random_planted(dtype, rng):
    """a few paths of random length: straight pieces with corners, noise, and here and there a wild value"""
    paths = []
    for _ in range(int(rng.integers(1, 5))):
        n = int(rng.integers(1, 70))
        pts, x, y = [], float(rng.uniform(-60, 60)), float(rng.uniform(-40, 40))
        dx, dy = rng.uniform(-1.5, 1.5, 2)
        for i in range(n):
            if rng.random() < 0.06:
                dx, dy = rng.uniform(-1.5, 1.5, 2)
            x, y = x + dx, y + dy
            pts.append((x + rng.normal(0, 0.2), y + rng.normal(0, 0.2)))
        paths.append(pts)
    kl = keylines_on_paths(dtype, paths, extra=int(rng.integers(0, 4)))
    n = len(kl)
    kl["rho"] = rng.uniform(0.05, 3.0, n).astype(F32)
    kl["sigma_rho"] = (kl["rho"] * rng.uniform(0.0, 0.6, n).astype(F32)).astype(F32)
    kl["matches"] = rng.integers(1, 6, n)
    for k in np.flatnonzero(rng.random(n) < 0.02):
        kl["pos_img"][k, int(rng.integers(0, 2))] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30], F32))
    for k in np.flatnonzero(rng.random(n) < 0.02):
        kl["sigma_rho"][k] = rng.choice(np.array([0.0, -0.01, 1e-9], F32))
    return kl
