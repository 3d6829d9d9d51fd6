"""What more than one test file uses: constants, bit-level comparison, the numpy reference models the GPU tests compare against
(and the CPU tests check by hand), the crafted forwardMatch maps, stream and pair drivers, the handles and sentences of the
refusal tables, and the backend / B / host_lib / refusal_scene fixtures.

A plain module, importable as `support` because tests/ is on the path; importing it needs no GPU (torch and rebvio_amd.backend
are imported inside the functions and fixtures that use them). A test file takes a fixture with
`from support import B  # noqa: F401`: pytest finds it in the importing module, one instance per test module.
Helpers and configurations of a single file stay in that file; no test file imports another (tests/test_support_layout.py)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import params_for

# ---- constants ----------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "rebvio_amd", "_build")
INC = ["-I", os.path.join(ROOT, "include")]
F32 = np.float32
TS = 50000                       # microseconds between frames: frame_dt = 0.05 on both APIs
EUROC_D = [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0]  # camera.hpp:31-35
KW_C2 = dict(keylines_ref=15000, keylines_max=16000)   # the bench configuration of the 640x480 stream
KW_TRACK = dict(keylines_ref=1500, keylines_max=2500, global_min_matches_threshold=1)   # the 192x144 stream of the tracking tests
RHO_MIN, RHO_MAX = np.float32(1e-3), np.float32(20.0)  # types/keyline.hpp:13-14
GRAY8, RGB8, BGR8, RGBA8, BGRA8, YUYV, UYVY = range(7)   # REBVIO_HIP_PX_*
NAMES = ["GRAY8", "RGB8", "BGR8", "RGBA8", "BGRA8", "YUYV", "UYVY"]
BPP = (1, 3, 3, 4, 4, 2, 2)
DF_TILE, DF_MAX_TILES, DF_TILE_CAP = 32, 4096, 512   # kDfTile, kDfMaxTiles, kDfTileCap (rebvio_amd/csrc/common.hpp)
CLOUD_DTYPE = np.dtype([("xyz", "<f4", (3,)), ("rho", "<f4"), ("sigma_rho", "<f4"), ("gradient_norm", "<f4"),
                        ("keyline", "<i4"), ("matches", "<u4")])
IDENTITY = (np.eye(3, dtype=F32), np.zeros(3, F32), F32(1.0))
KF_MATCH_DTYPE = np.dtype([("kf_keyline", "<i4"), ("keyline", "<i4"), ("claimants", "<i4"), ("matches", "<u4"), ("rho", "<f4"),
                           ("sigma_rho", "<f4"), ("pos_img", "<f4", (2,))])
# (REBVIO_HIP_LM, REBVIO_HIP_LM_THREADS, REBVIO_HIP_DM_HEAD): every LM kernel form and workgroup size, the other two directedMatch forms
FORMS = [(lm, th, None) for lm in (None, "seq", "percall", "spec3") for th in (256, 512, 1024)] + [(None, None, "compact4"), (None, None, "compact1")]


# ---- bit-level comparison -----------------------------------------------------------------------------------------------
def f32(x):
    return np.float32(x)


def bits_equal(a, b):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    if a.dtype.kind == "f":
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)


def words(a):
    """fp32 values as raw words, a NaN counted as a NaN (as record_words)"""
    a = np.array(a, np.float32).reshape(-1)
    a[np.isnan(a)] = np.float32(np.nan)
    return a.view(np.uint32)


def record_words(po):
    """every field of a pair record as raw 32-bit words (floats by their bits)"""
    out = []
    for name, _ in type(po)._fields_:
        v = getattr(po, name)
        a = np.array(v) if hasattr(v, "__len__") else np.array([v])
        if a.dtype.kind == "f":
            a = a.astype(np.float32)
            a[np.isnan(a)] = np.float32(np.nan)  # (a NaN is a NaN: sign and payload of one are not part of the result)
            out.append(a.view(np.uint32))
        else:
            out.append(a.astype(np.int64).astype(np.uint32))
    return np.concatenate(out)


def rec(out, n):
    """a pair record's words, then the keyline count that came with it"""
    return np.append(record_words(out), np.uint32(n))


def state_words(st):
    return np.concatenate([np.asarray(st[0], np.float32).view(np.uint32), np.asarray(st[1], np.float32).reshape(-1).view(np.uint32)])


def same_records(a, b, what):
    assert len(a) == len(b), (what, len(a), len(b))
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), (what, k, np.flatnonzero(x != y)[:8])


def assert_keylines_equal(ko, kg, what="", skip=()):
    """every field of two keyline arrays but those of `skip`, floats by their bits"""
    assert len(ko) == len(kg), f"{what}: size {len(ko)} vs {len(kg)}"
    for f in ko.dtype.names:
        if f in skip:
            continue
        if not bits_equal(ko[f], kg[f]):
            bad = np.nonzero((ko[f] != kg[f]).reshape(len(ko), -1).any(1))[0]
            raise AssertionError(f"{what}: field {f} differs at {len(bad)} keylines, first {bad[:5]}: "
                                 f"{ko[f][bad[:3]]} vs {kg[f][bad[:3]]}")


def nan_canonical(kl):
    """keylines with every NaN of a float field replaced by the one quiet NaN (as record_words does for records)"""
    kl = kl.copy()
    for f in kl.dtype.names:
        if kl.dtype[f].base.kind == "f":
            a = kl[f]
            a[np.isnan(a)] = np.float32(np.nan)
    return kl


def assert_keylines_equal_nan(ko, kg, what=""):
    assert_keylines_equal(nan_canonical(ko), nan_canonical(kg), what=what)


# ---- numpy reference models ---------------------------------------------------------------------------------------------
# the point cloud (include/rebvio_hip.h; checked by hand in tests/test_point_cloud.py)
def np_passes(kl, min_matches, max_rel_sigma, rho_min, rho_max):
    """The filter: positive tests (a NaN fails them); sigma_rho <= max_rel_sigma * rho with one rounded fp32 multiply."""
    rho, sig = kl["rho"].astype(F32), kl["sigma_rho"].astype(F32)
    with np.errstate(all="ignore"):
        bound = (F32(max_rel_sigma) * rho).astype(F32)
        return (kl["matches"] >= np.uint32(min_matches)) & (rho >= F32(rho_min)) & (rho <= F32(rho_max)) & (sig <= bound)


def np_cloud(kl, fm, flt, pose=None):
    """flt = (min_matches, max_rel_sigma, rho_min, rho_max); pose = (R[3, 3], t[3], scale) or None. Returns CLOUD_DTYPE records in
    ascending keyline index."""
    R, t, scale = IDENTITY if pose is None else pose
    R = np.asarray(R, F32).reshape(9)
    t = np.asarray(t, F32).reshape(3)
    idx = np.flatnonzero(np_passes(kl, *flt))
    k = kl[idx]
    out = np.zeros(len(idx), CLOUD_DTYPE)
    fm = F32(fm)
    with np.errstate(all="ignore"):
        u = (k["pos_img"][:, 0].astype(F32) / fm).astype(F32)
        v = (k["pos_img"][:, 1].astype(F32) / fm).astype(F32)
        z = (F32(scale) / k["rho"].astype(F32)).astype(F32)
        xc, yc = (u * z).astype(F32), (v * z).astype(F32)
        for i in range(3):
            a = ((R[3 * i] * xc).astype(F32) + (R[3 * i + 1] * yc).astype(F32)).astype(F32)
            b = (a + (R[3 * i + 2] * z).astype(F32)).astype(F32)
            out["xyz"][:, i] = (b + t[i]).astype(F32)
    out["rho"], out["sigma_rho"], out["gradient_norm"] = k["rho"], k["sigma_rho"], k["gradient_norm"]
    out["keyline"], out["matches"] = idx, k["matches"]
    return out


# keyframe correspondences (checked by hand in tests/test_keyframe.py)
def np_kf_matches(kl, kf_size):
    """rebvio_hip_map_keyframe_matches on a KEYLINE_DTYPE array: (records in ascending kf_keyline, their number). Keyline i claims
    slot j = match_id_keyframe[i] when 0 <= j < kf_size; per slot the claimant of smallest (sk << 32) | i wins, sk = bits of
    sigma_rho + 0.0f when sigma_rho >= 0, 0xFFFFFFFF otherwise."""
    ids = kl["match_id_keyframe"].astype(np.int64)
    sr = np.ascontiguousarray(kl["sigma_rho"], F32)
    ok = (ids >= 0) & (ids < kf_size)
    with np.errstate(invalid="ignore"):
        ordered = sr >= 0
        sk = np.where(ordered, (sr + F32(0.0)).view(np.uint32), np.uint32(0xFFFFFFFF)).astype(np.uint64)
    key = (sk << np.uint64(32)) | np.arange(len(kl), dtype=np.uint64)
    slots = np.unique(ids[ok])
    out = np.zeros(len(slots), KF_MATCH_DTYPE)
    for r, j in enumerate(slots):
        cl = np.flatnonzero(ok & (ids == j))
        w = cl[np.argmin(key[cl])]
        out[r]["kf_keyline"], out[r]["keyline"], out[r]["claimants"] = j, w, len(cl)
        for f in ("matches", "rho", "sigma_rho", "pos_img"):
            out[r][f] = kl[w][f]
    return out, len(slots)


# the oracle's distance-field rule, per tile (checked in tests/test_envelope_inputs.py)
def df_tile_edge(rows, cols):
    """df_grid (common.hpp): the tile edge doubles while the frame has more than kDfMaxTiles tiles"""
    T = DF_TILE
    while -(-cols // T) * -(-rows // T) > DF_MAX_TILES:
        T *= 2
    return T


def _round_half_away(x):
    """std::round of fp32 values (get_index, oracle/rebvio_oracle.cpp), as integers"""
    x = x.astype(np.float64)  # |x| + 0.5 is exact in double for every fp32 in the range of an image
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)


def tile_lower_bounds(kl, threshold, rows, cols, search_range, T):
    """[nty, ntx]: the number of distinct keylines that write at least one cell of each T x T tile by the rule of
    orc_build_distance_field - for r in [-search_range, search_range): cell get_index(pos + r * gradient / gradient_norm), fp32
    operation by operation, keylines under the map's threshold skipped. Every such keyline has to be in the device's list
    of that tile (or its field would be wrong), so this is a lower bound of the device's tile_cnt."""
    ntx, nty = -(-cols // T), -(-rows // T)
    thr = np.float32(threshold)
    gn = kl["gradient_norm"].astype(np.float32)
    keep = ~((thr > 0) & (gn < thr))
    idx = np.flatnonzero(keep)
    counts = np.zeros(nty * ntx, np.int64)
    r = np.arange(-int(search_range), int(search_range), dtype=np.int64).astype(np.float32)[None, :]
    for lo in range(0, len(idx), 8192):
        sel = idx[lo:lo + 8192]
        k = kl[sel]
        ux = (k["gradient"][:, 0] / gn[sel]).astype(np.float32)[:, None]
        uy = (k["gradient"][:, 1] / gn[sel]).astype(np.float32)[:, None]
        fr = (uy * r).astype(np.float32) + k["pos"][:, 1].astype(np.float32)[:, None]
        fc = (ux * r).astype(np.float32) + k["pos"][:, 0].astype(np.float32)[:, None]
        row, col = _round_half_away(fr), _round_half_away(fc)
        ok = (row >= 0) & (row < rows) & (col >= 0) & (col < cols)
        tile = (row // T) * ntx + col // T
        key = (np.arange(len(sel), dtype=np.int64)[:, None] * (ntx * nty) + tile)[ok]
        counts += np.bincount(np.unique(key) % (ntx * nty), minlength=ntx * nty)
    return counts.reshape(nty, ntx)


def assert_crowded_and_sparse(om, rows, cols, search_range=40, what=""):
    """The precondition of the crowded-tile tests, on the oracle's map alone: some tile is certainly over the list capacity
    (lower bound > 512: rebuilt from the row range) and some non-empty tile is certainly under it (the device's count can
    exceed the lower bound - its clip adds a cell each side - so the margin is a factor of two: <= 256)."""
    T = df_tile_edge(rows, cols)
    lb = tile_lower_bounds(om.keylines(), om.threshold, rows, cols, search_range, T)
    assert lb.max() > DF_TILE_CAP, f"{what}: no tile over the cap (T = {T}, peak {lb.max()})"
    assert ((lb > 0) & (lb <= DF_TILE_CAP // 2)).any(), f"{what}: no non-empty tile certainly on the list path"
    return lb


def half_pixel_keylines(kl, W, H):
    """kl (at least 48 keylines of a W x H frame) with its first 48 keylines moved onto half-integer positions at and near the four borders, gradients along the axes: every
    cell coordinate pos + r * unit is then a tie of std::round (getIndex, core.hpp:66-71), -0.5 (which rounds away from zero, out of
    the image) and rows - 0.5 / cols - 0.5 among them."""
    out = kl.copy()
    k = np.arange(48)
    side = k % 4
    along = (5 + 3 * (k // 4)).astype(np.float32) + np.float32(0.5)
    x = np.where(side == 0, 0.5, np.where(side == 1, W - 1.5, along)).astype(np.float32)
    y = np.where(side == 2, 0.5, np.where(side == 3, H - 1.5, along)).astype(np.float32)
    g = (1.0 + 0.25 * (k % 5)).astype(np.float32)
    out["pos"][:48, 0], out["pos"][:48, 1] = x, y
    out["gradient"][:48, 0] = np.where(side < 2, np.where(k % 8 < 4, g, -g), 0)
    out["gradient"][:48, 1] = np.where(side >= 2, np.where(k % 8 < 4, g, -g), 0)
    out["gradient_norm"][:48] = g
    return out


def noise_frames(W, H, n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, H, W)).astype(np.uint8)


# rotations and streams
def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.sqrt((w * w).sum())
    if th == 0:
        return np.eye(3)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    return np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / (th * th)) * (K @ K)


def gyro_rotations(order, seed, stream_id=0):
    """One rotation per frame of order[]: [k] spans frame order[k-1] -> order[k]. [0] belongs to no pair (the drivers ignore a
    first frame's rotation): a rotation of its own, far from the identity, so that using it anywhere shows."""
    from rebvio_amd import synth
    scene = synth.make_scene(stream_id, 1.0)
    rng = np.random.Generator(np.random.PCG64(seed))
    out = [rodrigues([0.3, -0.2, 0.1]).astype(np.float32)]
    for i, j in zip(order[:-1], order[1:]):
        Ri, Rj = synth.pose(scene, int(i))[0], synth.pose(scene, int(j))[0]
        w = rng.uniform(-0.004, 0.004, 3)
        out.append(((Ri.T @ Rj).T @ rodrigues(w)).astype(np.float32))
    return out


def enlarged_stream(width, height, n, factor=4, **kw):
    """n frames of a synth stream rendered at 1/factor of the size and enlarged (every pixel a factor x factor block), cut to
    width x height; the camera of the enlarged frames (pixel (x, y) covers x*f .. x*f + f-1: centre x*f + (f-1)/2)."""
    from rebvio_amd import synth
    qw, qh = -(-width // factor), -(-height // factor)
    small, qcam = synth.render_stream(qw, qh, n, **kw)
    big = np.kron(small, np.ones((1, factor, factor), np.uint8))[:, :height, :width]
    off = 0.5 * (factor - 1)
    return np.ascontiguousarray(big), synth.Camera(width, height, qcam.fm * factor, qcam.cx * factor + off, qcam.cy * factor + off)


def c2_order():
    """sixteen frames, back and forth over the eight of c2_stream"""
    from rebvio_amd import synth
    return synth.pingpong_indices(8, 16)


def vision_only_fusion(mid):
    """rebvio.cpp:195-203,225-233 without the inertial filter, in numpy (it only has to be the same in every run compared)."""
    Xgv = np.array(mid.Xgv, np.float64)
    R = np.array(mid.R, np.float64).reshape(3, 3)
    w = Xgv[3:]
    th = np.linalg.norm(w)
    if th > 0:
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
        R0 = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    else:
        R0 = np.eye(3)
    R = (R0 @ R.T).T
    V = R0 @ np.array(mid.Vg, np.float64) + Xgv[:3]
    P = np.linalg.inv(np.array(mid.W_Xgv, np.float64).reshape(6, 6))[:3, :3]
    return V.astype(F32), P.astype(F32), R.astype(F32), R0.astype(F32)


# colour frames
def luma(rgb):
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


def colourise(grey, seed):
    """grey [n, H, W] -> {fmt: (frames [n, H, W, bpp] or [n, H, W], the grey frames the grey path gets)}"""
    rng = np.random.default_rng(seed)
    n, H, W = grey.shape
    g = grey.astype(np.int16)
    yy, xx = np.mgrid[0:H, 0:W]
    smooth = (40 * np.sin(xx / 37.0) * np.cos(yy / 23.0)).astype(np.int16)             # smooth chroma
    rgb = np.stack([g + rng.integers(-40, 41, g.shape, dtype=np.int16),                 # random per-pixel chroma
                    g + smooth[None],
                    g - smooth[None] + rng.integers(-25, 26, g.shape, dtype=np.int16)], -1)
    rgb = np.clip(rgb, 0, 255).astype(np.uint8)
    alpha = rng.integers(0, 256, (n, H, W, 1), dtype=np.uint8)
    grey_rgb = luma(rgb)
    chroma = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    return {
        GRAY8: (grey, grey),
        RGB8: (rgb, grey_rgb),
        BGR8: (np.ascontiguousarray(rgb[..., ::-1]), grey_rgb),
        RGBA8: (np.concatenate([rgb, alpha], -1), grey_rgb),
        BGRA8: (np.concatenate([rgb[..., ::-1], alpha], -1), grey_rgb),
        YUYV: (np.stack([grey, chroma], -1), grey),      # bytes Y0 U Y1 V
        UYVY: (np.stack([chroma, grey], -1), grey),      # bytes U Y0 V Y1
    }


# the masked detector, from the oracle's unmasked map
def join_edges(kl, dense):
    """EdgeDetector::joinEdges / nextKeylineIdx (edge_detector.cpp:124-165) over the keylines kl and their dense index mask"""
    kl["id_prev"] = -1
    kl["id_next"] = -1
    if len(kl) == 0:
        return
    pos = kl["pos"].astype(np.float64)
    x = (pos[:, 0] + 0.5).astype(np.int64)
    y = (pos[:, 1] + 0.5).astype(np.int64)
    tx, ty = -kl["gradient"][:, 1], kl["gradient"][:, 0]
    sx = np.where(ty > 0, np.where(tx > 0, 1, -1), np.where(tx < 0, -1, 1))
    sy = np.where(ty > 0, 1, -1)
    c1, c2, c3 = dense[y, x + sx], dense[y + sy, x], dense[y + sy, x + sx]
    nxt = np.where(c1 >= 0, c1, np.where(c2 >= 0, c2, np.where(c3 >= 0, c3, -1)))
    kl["id_next"] = nxt
    prev = kl["id_prev"]
    for idx, j in enumerate(nxt.tolist()):   # in index order: a later keyline overwrites id_prev
        if j >= 0:
            prev[j] = idx


def tune_threshold(kl, previous):
    """tuneThreshold (edge_detector.cpp:167-186) with size <= keylines_max: the cumulative loop ends at i = num_bins"""
    if len(kl) == 0:
        return np.float32(previous)
    g = kl["gradient_norm"]
    mx, mn = g.max(), g.min()
    return np.float32(mx - np.float32(np.float32(100) * (mx - mn)) / np.float32(100))


def masked_map(om, H, W, keep, kmax, previous_auto):
    """(keylines, dense mask, map threshold) the masked detector must produce, from the oracle's unmasked map om"""
    kl = om.keylines()
    dense = om.mask(H, W).ravel()
    pix = np.full(len(kl), -1, np.int64)
    at = np.flatnonzero(dense >= 0)
    pix[dense[at]] = at                         # each keyline's pixel
    assert (pix >= 0).all() and (np.diff(pix) > 0).all()
    sel = keep.ravel()[pix] != 0
    kl, pix = kl[sel][:kmax].copy(), pix[sel][:kmax]
    d2 = np.full(H * W, -1, np.int32)
    d2[pix] = np.arange(len(kl), dtype=np.int32)
    d2 = d2.reshape(H, W)
    join_edges(kl, d2)
    return kl, d2, tune_threshold(kl, previous_auto)


def assert_map(want, gm, what):
    kl, dense, thr = want
    assert gm.size() == len(kl), (what, gm.size(), len(kl))
    assert_keylines_equal(kl, gm.keylines(), what=what)
    assert np.array_equal(gm.mask(), dense), what
    assert bits_equal(np.float32(gm.threshold), thr), (what, gm.threshold, thr)


# ---- crafted forwardMatch maps (tests/test_forward_match.py states the rule; each helper asserts what its map claims) ---
GROUP_SIZES = (1, 2, 3, 63, 64, 65, 256, 257, 600)
N_FILL = 120           # further groups of 1, 2 and 3 writers: enough targets for every pre-set kind of section b
LAYOUTS = ("contiguous", "stride6")
PATTERNS = ("distinct", "equal", "shared_max", "clamps")
PRESETS = ("above", "equal", "ulp_above", "ulp_below", "well_below")   # the target's own rho against the winning writer's
WG = 256               # threads per workgroup of k_forward_keys; the LM kernels publish from 256, 512 or 1024
HANDED = ("rho", "sigma_rho", "matches", "match_id", "match_pos_img", "match_gradient", "match_gradient_norm", "match_id_keyframe")


def ulp_up(x):
    return np.nextafter(f32(x), f32(np.inf), dtype=np.float32)


def ulp_down(x):
    return np.nextafter(f32(x), f32(-np.inf), dtype=np.float32)


def writers_by_target(old):
    """dict target -> ascending old indices whose match_id_forward names it"""
    fwd = old["match_id_forward"]
    w = np.flatnonzero(fwd >= 0)
    order = np.argsort(fwd[w], kind="stable")
    w = w[order]
    cuts = np.flatnonzero(np.diff(fwd[w])) + 1
    return {int(fwd[g[0]]): g for g in np.split(w, cuts)} if len(w) else {}


def winner_of(old, members):
    """the writer of largest rho, the largest index among equals"""
    rho = old["rho"][members]
    return int(members[np.flatnonzero(rho == rho.max())[-1]])


def forward_match_closed_form(old, new):
    """(the new map after old->forwardMatch(new), the returned count), from the rule in the docstring of tests/test_forward_match.py"""
    out = new.copy()
    count = 0
    for t, members in writers_by_target(old).items():
        rho = old["rho"][members]
        matched = new["match_id"][t] >= 0
        front = np.maximum.accumulate(np.concatenate([[new["rho"][t] if matched else f32(-np.inf)], rho]))[:-1]
        count += int((rho >= front).sum())
        w = winner_of(old, members)
        if matched and new["rho"][t] > old["rho"][w]:
            continue
        out["rho"][t] = old["rho"][w]
        out["sigma_rho"][t] = old["sigma_rho"][w]
        out["matches"][t] = old["matches"][w] + np.uint32(1)
        out["match_id"][t] = w
        out["match_pos_img"][t] = old["pos_img"][w]
        out["match_gradient"][t] = old["gradient"][w]
        out["match_gradient_norm"][t] = old["gradient_norm"][w]
        out["match_id_keyframe"][t] = old["match_id_keyframe"][w]
    return out, count


def group_slots(n_old, layout):
    """Old indices in the order the groups take them, index 0 and n_old - 1 kept back for the two sole writers. stride6: the
    indices of one residue class mod 6 after the other, so that consecutive members of a group lie six apart. A class of this
    map holds n_old / 6 indices, fewer than the 600 (and, behind it, the 257 and 256) writers ask for: such a group goes on in
    the next class, still six apart, and reaches over every workgroup of the map."""
    idx = np.arange(1, n_old - 1)
    if layout == "stride6":
        idx = np.concatenate([idx[idx % 6 == r] for r in range(6)])
    return idx


def group_rhos(pattern, g, size, rng):
    """rho of the `size` writers of group number g, in member order"""
    k = np.arange(size)
    base = f32(0.5) + f32(0.125) * f32(g % 5)
    if pattern == "equal":
        return np.full(size, base, np.float32)
    distinct = (base + f32(2.0 ** -10) * rng.permutation(size).astype(np.float32)).astype(np.float32)
    if pattern == "distinct":
        return distinct
    if pattern == "shared_max":   # the maximum twice, in the first and in the last quarter of the group (once in a group of one)
        top = f32(distinct.max() + f32(0.25))
        distinct[size // 8] = top
        distinct[size - 1 - size // 8] = top
        return distinct
    assert pattern == "clamps"
    if g % 4 == 0:      # every writer at kRhoMin: the smallest key of the claimed range wins
        return np.full(size, RHO_MIN, np.float32)
    if g % 4 == 1:      # every writer at kRhoMax
        return np.full(size, RHO_MAX, np.float32)
    if g % 4 == 2:      # both clamps among natural values: the last writer at kRhoMax wins
        return np.where(k % 3 == 0, RHO_MAX, np.where(k % 3 == 1, RHO_MIN, distinct)).astype(np.float32)
    distinct[k % 2 == 1] = RHO_MIN   # every second writer at kRhoMin under a natural winner
    return distinct


def craft_writers(old, n_new, layout, pattern):
    """The old map with match_id_forward = -1 everywhere but for crafted groups of writers, one target each: GROUP_SIZES, N_FILL
    small groups, and old index 0 and n_old - 1 as sole writers (the low word of index 0's key is 0). Targets 0 and n_new - 1 are
    among the targets. Returns (old map, list of (target, member indices)); asserts what the layout claims."""
    old = old.copy()
    n_old = len(old)
    rng = np.random.default_rng(len(layout) * 100 + len(pattern))
    sizes = sorted(GROUP_SIZES, reverse=True) + [1 + (j // 4) % 3 for j in range(N_FILL)]
    slots = group_slots(n_old, layout)
    assert sum(sizes) <= len(slots), (sum(sizes), n_old)
    n_groups = len(sizes) + 2
    targets = np.unique(np.linspace(0, n_new - 1, n_groups).astype(int))
    assert len(targets) == n_groups and targets[0] == 0 and targets[-1] == n_new - 1
    targets = targets[rng.permutation(n_groups)]    # (no relation between a group's place in the old map and its target's)
    old["match_id_forward"] = -1
    old["matches"] = (np.arange(n_old) % 7).astype(np.uint32)   # (what a wrong winner hands over differs in every field)
    old["match_id_keyframe"] = np.arange(n_old) % 11 - 1
    groups, at = [], 0
    for g, size in enumerate(sizes + [1, 1]):
        if g < len(sizes):
            members = np.sort(slots[at:at + size])
            at += size
        else:
            members = np.array([0 if g == len(sizes) else n_old - 1])
        old["match_id_forward"][members] = targets[g]
        old["rho"][members] = group_rhos(pattern, g, size, rng)
        groups.append((int(targets[g]), members))
    # what the layout claims, on the crafted array
    by_target = writers_by_target(old)
    assert len(by_target) == n_groups and all(np.array_equal(by_target[t], m) for t, m in groups)
    assert (old["rho"] >= RHO_MIN).all() and (old["rho"] <= RHO_MAX).all()
    assert int(old["match_id_forward"][0]) >= 0 and int(old["match_id_forward"][n_old - 1]) >= 0
    for t, m in groups:
        if len(m) >= 256:
            assert len(np.unique(m // WG)) >= 2, (len(m), m[0], m[-1])
        if layout == "stride6" and len(m) > 1:
            classes = [m[m % 6 == r] for r in np.unique(m % 6)]   # six apart within a class, at most two classes (one wrap)
            assert len(classes) <= 2 and all((np.diff(c) == 6).all() for c in classes), m[:8]
        if pattern == "distinct":
            assert len(np.unique(old["rho"][m])) == len(m)
        if pattern == "shared_max" and len(m) >= 2:
            top = np.flatnonzero(old["rho"][m] == old["rho"][m].max())
            assert len(top) == 2
            if len(m) >= 256:
                assert m[top[0]] // WG != m[top[1]] // WG
    if pattern == "clamps":
        wins = np.array([old["rho"][winner_of(old, m)] for _, m in groups])
        assert (wins == RHO_MIN).sum() >= 10 and (wins == RHO_MAX).sum() >= 10
    return old, groups


def preset_targets(new, old, groups):
    """The new map with every target of `groups` already matched (match_id >= 0) and its rho set against the winning writer's:
    above, equal, one ulp above, one ulp below, well below (PRESETS in turn). edge_map.cpp:83 keeps the first and the third.
    Returns (new map, kind per group)."""
    new = new.copy()
    kinds = []
    n_old = len(old)
    for j, (t, m) in enumerate(groups):
        wr = old["rho"][winner_of(old, m)]
        kind = PRESETS[j % len(PRESETS)]
        if kind == "above" and wr == RHO_MAX:   # (nothing in the claimed range lies above kRhoMax)
            kind = "equal"
        if kind == "well_below" and wr == RHO_MIN:
            kind = "equal"
        if kind == "ulp_above" and wr == RHO_MAX:
            kind = "ulp_below"
        if kind == "ulp_below" and wr == RHO_MIN:
            kind = "ulp_above"
        new["rho"][t] = {"above": f32(min(wr * f32(1.5), RHO_MAX)), "equal": wr, "ulp_above": ulp_up(wr), "ulp_below": ulp_down(wr),
                         "well_below": f32(max(wr * f32(0.5), RHO_MIN))}[kind]
        new["match_id"][t] = (7 * j + 3) % n_old
        new["sigma_rho"][t] = f32(0.0625) * f32(1 + j % 9)
        new["matches"][t] = 100 + j
        new["match_pos_img"][t] = (f32(j) - f32(40.5), f32(30.25) - f32(j))
        new["match_gradient"][t] = (f32(1.5), f32(-2.0))
        new["match_gradient_norm"][t] = f32(2.5)
        new["match_id_keyframe"][t] = j % 3 - 1
        kinds.append(kind)
    assert (new["rho"] >= RHO_MIN).all() and (new["rho"] <= RHO_MAX).all()
    return new, kinds


def kept_and_overwritten(before, after, groups):
    """(targets that kept every bit, targets that were overwritten), from a result alone"""
    kept = over = 0
    for t, _ in groups:
        same = all(np.array_equal(np.ascontiguousarray(before[f][t:t + 1]).view(np.uint32), np.ascontiguousarray(after[f][t:t + 1]).view(np.uint32))
                   for f in HANDED)
        kept, over = kept + same, over + (not same)
    return kept, over


def drop_every_second_writer(old):
    """the old map with match_id_forward = -1 on every second writer (in index order over all writers)"""
    old = old.copy()
    w = np.flatnonzero(old["match_id_forward"] >= 0)
    old["match_id_forward"][w[1::2]] = -1
    return old


# start velocities of minimizeVel and the accept masks the oracle gives for them on the stage's pair (iteration 0 is the last
# digit); the second and third are the second runs of section c
START_VELS = (((0.05, 0.0, 0.0), "00001"), ((0.0, 0.0, -0.06), "00001"), ((0.2, 0.1, 0.0), "01111"), ((0.0, 0.0, -0.9), "01111"))
RERUN_VELS = (START_VELS[1][0], START_VELS[2][0])


def targets_of(kl):
    f = kl["match_id_forward"]
    return set(f[f >= 0].tolist())


def behind_the_camera(kl, threshold, sigma_rho_min, vz):
    """keylines that tryVel evaluates (core.cpp:88-91) and that take its z_p <= 0 branch (core.cpp:96-98) at forward speed vz"""
    z_p = (1.0 / kl["rho"].astype(np.float64) + vz).astype(np.float32)
    return int(((kl["gradient_norm"] >= threshold) & (kl["sigma_rho"] <= sigma_rho_min) & (z_p <= 0)).sum())


DONOR = 936            # a well-matched keyline of the old map of the stage's pair (frames 3 -> 4)
DONOR_COPIES = 300     # old keylines 3, 9, 15, ... made copies of one well-matched donor
DONOR_FIELDS = ("pos", "pos_img", "gradient", "gradient_norm", "rho", "sigma_rho", "matches")


def craft_donor_copies(old, donor, varied):
    """Section e: DONOR_COPIES old keylines (3, 9, 15, ...) made copies of keyline `donor` in the fields tryVel reads, so that all
    of them forward to the donor's target through a whole pair. varied: rho * (1 + (k % 37 - 18) * 2^-14) on copy k - the
    maximum (k % 37 == 36) is shared by several copies."""
    old = old.copy()
    idx = 3 + 6 * np.arange(DONOR_COPIES)
    assert idx[-1] < len(old) and donor not in idx
    for f in DONOR_FIELDS:
        old[f][idx] = old[f][donor]
    if varied:
        k = np.arange(DONOR_COPIES)
        old["rho"][idx] = (old["rho"][donor] * (f32(1) + (k % 37 - 18).astype(np.float32) * f32(2.0 ** -14))).astype(np.float32)
        assert (old["rho"][idx] == old["rho"][idx].max()).sum() >= 2
    return old, idx


def assert_donor_pair(po, old_after, idx, varied):
    """Section e on the oracle's result alone: the pair tracks, one target has at least 257 writers from at least 2 workgroups
    (of 256 keylines, the smallest the kernels use), and the winner the crafted rhos call for."""
    assert po.status == 0, po.status
    t, m = max(writers_by_target(old_after).items(), key=lambda kv: len(kv[1]))
    assert len(m) >= 257 and len(np.unique(m // WG)) >= 2 and len(np.unique(m // 1024)) >= 2, (t, len(m))
    assert winner_of(old_after, m) == (1773 if varied else 1797)
    return t, m


# ---- stream and pair drivers --------------------------------------------------------------------------------------------
# frame stamps off the one interval TS (tests/test_frame_interval_gpu.py, tests/test_reference_pin.py): the steps in microseconds
# between the twelve frames of small_stream. On the CPU oracle (KW_TRACK, sums in device order) all eleven pairs end with status 0.
STEPS_HEALTHY = (50000, 33333, 33334, 100000, 20000, 5000, 1000000, 40000, 1000, 200000, 50000)
EUROC_T0 = 1403636579763555      # an absolute stamp of the size EuRoC's are
# the frame intervals (s) the gyroBiasCorrection cases run at: the last two are a repeated stamp and a stamp that goes back by
# 40 ms (the uint64 difference as a float)
DT_GRID = (1, 0.2, 0.1, 0.05, 0.0333333, 0.02, 0.005, 0.001, 2e-4, 1.9e-4, 1.5e-4, 1e-6, 0, 1.8446744e13)


def stamps_from(steps, t0=0):
    """frame stamps (python ints, microseconds): t0, then one step further per frame"""
    out = [int(t0)]
    for d in steps:
        out.append(out[-1] + int(d))
    return out


def default_stamps(n, stamps=None):
    """the stamps of n frames: k * TS unless a list is given"""
    if stamps is None:
        return [k * TS for k in range(n)]
    assert len(stamps) == n, (len(stamps), n)
    return [int(t) for t in stamps]


def frame_dt_of(ts_old, ts_new):
    """The interval between two stamps as the reference forms it (rebvio.cpp:183): the uint64 difference (it wraps when the
    stamps go back), to float, divided by 1e6 in double, to float."""
    d = np.uint64((int(ts_new) - int(ts_old)) % (1 << 64))
    return float(np.float32(np.float64(np.float32(d)) / 1000000.0))


def gyro_noise(p, frame_dt):
    """(s_g, s_b): the diagonals of RGyro and RGBias (rebvio.cpp:186-187) in fp32, std_dev * std_dev * dt * dt from left to right;
    p: a parameter record of either library."""
    with np.errstate(all="ignore"):
        dt = F32(frame_dt)
        a, b = F32(p.gyro_std_dev), F32(p.gyro_bias_std_dev)
        return F32(F32(F32(a * a) * dt) * dt), F32(F32(F32(b * b) * dt) * dt)


# the input families of the glue probe (tests/test_parity_gpu.py: test_glue_probe_random_inputs), one fixed draw each; the last one
# runs at every decade of W_Bg
GLUE_FAMILIES = ("well-conditioned", "rank-deficient", "zero-rotation", "nan-entry", "wbg-decades")
WBG_DECADES = tuple(range(-2, 7))


def glue_family(name, decade=4):
    """One extRotVel system of a family, as the pair glue takes it and as gyroBiasCorrection takes it. Block records xrv[nb, 32]
    (21 upper-triangle sums, 6 of JtF, the count) for n_new keylines; Wx[6, 6] and X[6]: their sum in fp32 and the least-squares
    solution in double, rounded (the device forms its own from xrv); minimizeVel's vel and JtJ6; Bg; a symmetric W_Bg around
    10^decade; a prior rotation."""
    k = GLUE_FAMILIES.index(name)
    rng = np.random.default_rng(100 + k)
    n_new = 700 + 37 * k
    nb = (n_new + 255) // 256
    rows = rng.standard_normal((nb, 300, 6)) * np.array([400.0, 400.0, 200.0, 500.0, 500.0, 300.0])
    if name == "rank-deficient":
        rows[:, :, 5] = rows[:, :, 4] * 2.0
    if name == "zero-rotation":
        rows[:, :, 3:] = 0.0
    Y = rng.standard_normal((nb, 300)) * 0.3
    xrv = np.zeros((nb, 32), F32)
    iu = np.triu_indices(6)
    for b in range(nb):
        xrv[b, :21] = (rows[b].T @ rows[b])[iu]
        xrv[b, 21:27] = rows[b].T @ Y[b]
        xrv[b, 27] = 300
    if name == "nan-entry":
        xrv[0, 2] = np.nan
    acc = xrv.astype(np.float64).sum(0)
    Wx = np.zeros((6, 6))
    Wx[iu] = acc[:21]
    Wx = (Wx + np.triu(Wx, 1).T).astype(F32)
    with np.errstate(all="ignore"):
        X = (np.linalg.pinv(Wx.astype(np.float64)) @ acc[21:27] if np.isfinite(Wx).all() else np.full(6, np.nan)).astype(F32)
    J = rng.standard_normal((200, 3)) * [300.0, 300.0, 150.0]
    JtJ = J.T @ J
    W_Bg = np.eye(3) * 10.0 ** decade * rng.uniform(1, 3) + rng.standard_normal((3, 3)) * 1e-3
    return dict(xrv=xrv, n_new=n_new, Wx=Wx, X=X, vel=(rng.standard_normal(3) * 0.01).astype(F32),
                JtJ6=np.array([JtJ[0, 0], JtJ[1, 1], JtJ[2, 2], JtJ[0, 1], JtJ[0, 2], JtJ[1, 2]], F32),
                Bg=(rng.standard_normal(3) * 3e-4).astype(F32), W_Bg=((W_Bg + W_Bg.T) / 2).astype(F32),
                R_prior=rodrigues(rng.standard_normal(3) * 1e-2).astype(F32))


GLUE_GBC = os.path.join(ROOT, "tests", "golden", "glue_gbc_reference.npz")   # tests/golden/make_glue_gbc.py


def glue_family_cases():
    """(family, decade of W_Bg) for every case of the gyroBiasCorrection grids"""
    return [(f, 4) for f in GLUE_FAMILIES[:-1]] + [(GLUE_FAMILIES[-1], d) for d in WBG_DECADES]


def set_forms(monkeypatch, lm=None, threads=None, head=None, batch_head=None, **env):
    """The kernel forms a context reads when it is created, and any further variables by name (env); None = the library's default."""
    forms = dict(REBVIO_HIP_LM=lm, REBVIO_HIP_LM_THREADS=threads, REBVIO_HIP_DM_HEAD=head, REBVIO_HIP_BATCH_DM_HEAD=batch_head)
    for name, v in dict(forms, **env).items():
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def run_stream(ctx, dev, order, npx, k0=0, ts_step=50000, stamps=None):
    """Push order[] through the streaming driver and flush: every pair's (record, keyline count), in pair order - len(order) - 1
    of them. Records come back several pushes late (the pair step runs on the device from end to end, pairs are queued in
    groups and the host reads them up to fifteen pairs behind); the flush tracks the pairs not started yet and delivers the
    rest. stamps: one per frame, in place of (k0 + k) * ts_step."""
    recs = []
    for k, i in enumerate(order):
        out, n = ctx.push_frame_u8_device(dev + int(i) * npx, (k0 + k) * ts_step if stamps is None else int(stamps[k]))
        if out.status >= 0:
            recs.append((out, n))
    recs.extend(ctx.flush())
    return recs


def pair_tuple(out, n=None):
    t = (tuple(out.Vg), tuple(out.P_Vg), out.F, tuple(out.Xv), tuple(out.W_Xv), tuple(out.Xgv), tuple(out.V), tuple(out.R),
         tuple(out.P_V), out.sigma_rho_min, out.ext_ok, out.klm_num, out.kf_matches, out.reg_num, out.lm_accept_mask, out.status)
    return t if n is None else t + (n,)


class Pair:
    """Oracle and GPU contexts driven over the same frames; keeps the last two maps of each."""

    def __init__(self, O, B, frames, cam, **kw):
        self.O, self.B = O, B
        self.frames, self.cam = frames, cam
        self.orc = O.Oracle(params_for(O, cam, **kw))
        self.ctx = B.Context(params_for(B, cam, **kw))
        self.om = []
        self.gm = []

    def detect(self, i):
        om = self.orc.detect_u8(self.frames[i], i * 50000)
        gm = self.ctx.detect_u8(self.frames[i], i * 50000)
        self.om.append(om)
        self.gm.append(gm)
        if len(self.om) > 2:
            self.om.pop(0)
            self.gm.pop(0).release()
        return om, gm

    def sync_gpu_from_oracle(self):
        for om, gm in zip(self.om, self.gm):
            gm.upload(om.keylines())


def warm(O, B, frames, cam, n_pairs, **kw):
    """Run n_pairs oracle tracking steps so that depths/matches are realistic; the GPU only detects."""
    P = Pair(O, B, frames, cam, **kw)
    P.detect(0)
    for i in range(1, n_pairs + 1):
        P.detect(i)
        P.orc.track_pair(P.om[0], P.om[1])
    P.detect(n_pairs + 1)  # pair under test: om[0] (tracked once as "new"), om[1] fresh
    P.sync_gpu_from_oracle()
    return P


def matching_stage(O, B, stream, n_warm=3, **kw):
    """n_warm oracle pairs, then the pair under test up to forwardMatch on the oracle; both sides hold the oracle's maps."""
    frames, cam = stream
    P = warm(O, B, frames, cam, n_warm, **dict(KW_TRACK, **kw))
    om_old, om_new = P.om
    P.orc.build_distance_field(om_new)
    P.ctx.build_distance_field(P.gm[1])
    ro = P.orc.minimize_vel(om_old)
    P.orc.forward_match(om_old, om_new)
    P.sync_gpu_from_oracle()
    return P, ro


def set_new_map(P, kl):
    """the same crafted array into the newest map of both sides (true size, through rebvio_hip_map_upload)"""
    assert len(kl) == P.om[1].size()
    for f, n in (("id_prev", len(kl)), ("id_next", len(kl)), ("match_id", P.om[0].size())):  # (match_id: of the older map)
        assert (kl[f] >= -1).all() and (kl[f] < n).all(), f
    P.om[1].set_keylines(kl)
    P.gm[1].upload(kl)


def assert_pipeline_bit_identical(orc_mod, B, frames, cam, order, kw, min_klm, what, every_pair_tracks=False, expect_status=None,
                                  stamps=None):
    """frames[order] through the oracle (keyline sums in the kernels' order) and through the library, the state carried
    independently on both sides: every word of every pair record equal through the per-pair API and through the streaming
    driver, every keyline field of the newest map equal after the last pair. every_pair_tracks: a precondition on the oracle
    alone - each pair ends with status 0 and at least global_min_matches_threshold LM matches (a real pair, not a failure
    path); without it only the last pair is asked for motion and more than min_klm matches. expect_status: the oracle's pair
    statuses, one per pair - asked for in place of that closing condition, for streams whose pairs are meant to fail. stamps:
    one per frame in place of k * TS - the oracle and the per-pair API get frame_dt_of the pair's two stamps, the streaming
    driver the stamps alone. Returns the oracle's records as words."""
    W, H, npairs = cam.width, cam.height, len(order) - 1
    ts = default_stamps(len(order), stamps)
    p_o = params_for(orc_mod, cam, **kw)
    orc = orc_mod.Oracle(p_o)
    orc.set_sum_order("device")
    gpu = B.Context(params_for(B, cam, **kw))
    mo, mg, rec_o, status_o = [], [], [], []
    for k, i in enumerate(order):
        mo.append(orc.detect_u8(frames[i], ts[k]))
        mg.append(gpu.detect_u8(frames[i], ts[k]))
        if len(mo) > 2:
            mo.pop(0)
            mg.pop(0).release()
        if k == 0:
            continue
        dt = frame_dt_of(ts[k - 1], ts[k])
        po = orc.track_pair(mo[0], mo[1], frame_dt=dt)
        if every_pair_tracks:
            assert po.status == 0 and po.klm_num >= p_o.global_min_matches_threshold, (what, k, po.status, po.klm_num)
        pg = gpu.track_pair(mg[0], mg[1], frame_dt=dt)
        wo, wg = record_words(po), record_words(pg)
        assert np.array_equal(wo, wg), (what, k, np.flatnonzero(wo != wg)[:8], np.array(po.Vg), np.array(pg.Vg))
        rec_o.append(wo)
        status_o.append(po.status)
    if expect_status is None:
        assert rec_o[-1][0] != 0 and po.klm_num > min_klm
    else:
        assert status_o == list(expect_status), (what, status_o)
    # the map that carries the state into the next pair (the older one is dropped after its pair, rebvio.cpp:136-139)
    assert_keylines_equal(mo[1].keylines(), mg[1].keylines(), what=f"{what}: newest map after {npairs} pairs")
    gpu.close()
    # the streaming driver on the same frames: device glue, persistent speculative LM kernel, pairs queued in groups
    ctx = B.Context(params_for(B, cam, **kw))
    dev = ctx.upload_frames(frames)
    got = []
    for k, i in enumerate(order):
        out, _ = ctx.push_frame_u8_device(dev + int(i) * W * H, ts[k])
        if out.status >= 0:
            got.append(record_words(out))
    for out, _ in ctx.flush():
        got.append(record_words(out))
    ctx.close()
    assert len(got) == len(rec_o) == npairs
    for k, (wo, wg) in enumerate(zip(rec_o, got)):
        assert np.array_equal(wo, wg), (what, k, np.flatnonzero(wo != wg)[:8])
    return rec_o


# ---- the three runners of a stream with per-frame rotations: oracle, per-pair API, streaming driver -----------------------
def oracle_pairs(orc_mod, cam, seq, R, keep=(), stamps=None, **kw):
    """seq[] through the CPU oracle alone, keyline sums in the kernels' order; R = None: no priors. (records, keyline counts);
    keep: pair numbers after which the keylines of both maps are kept - [(records, keyline counts), {pair: (old, new)}];
    stamps: one per frame in place of k * TS, every pair run at frame_dt_of its two stamps"""
    orc = orc_mod.Oracle(params_for(orc_mod, cam, **kw))
    orc.set_sum_order("device")
    ts = default_stamps(len(seq), stamps)
    recs, prev, kept = [], None, {}
    for k, f in enumerate(seq):
        m = orc.detect_u8(f, ts[k])
        if prev is not None:
            recs.append((orc.track_pair(prev, m, R_prior=None if R is None else R[k], frame_dt=frame_dt_of(ts[k - 1], ts[k])), m.size()))
            if k - 1 in keep:
                kept[k - 1] = (prev.keylines(), m.keylines())
        prev = m
    return (recs, kept) if keep else recs


def lib_pairs(B, cam, seq, R, mask=None, keep=(), stamps=None, **kw):
    """per-pair API: detect (+ per-frame mask) and rebvio_hip_track_pair(R_prior = R[k]); (records as words, gyro state);
    keep: as oracle_pairs - (records as words, gyro state, {pair: (old, new)}); stamps: as oracle_pairs"""
    ctx = B.Context(params_for(B, cam, **kw))
    ts = default_stamps(len(seq), stamps)
    npx = cam.width * cam.height
    dev = ctx.upload_frames(seq)
    mdev = ctx.upload_frames(mask[None]) if mask is not None else None
    maps, recs, kept = [], [], {}
    for k in range(len(seq)):
        if mdev is None:
            maps.append(ctx.detect_u8_device(dev + k * npx, ts[k]))
        else:
            maps.append(ctx.detect_px_masked_device(dev + k * npx, B.PX_GRAY8, mdev, ts[k]))
        if len(maps) > 2:
            maps.pop(0).release()
        if k:
            recs.append(rec(ctx.track_pair(maps[0], maps[1], R_prior=None if R is None else R[k], frame_dt=frame_dt_of(ts[k - 1], ts[k])),
                            maps[1].size()))
            if k - 1 in keep:
                kept[k - 1] = (maps[0].keylines(), maps[1].keylines())
    st = ctx.gyro_state()
    ctx.close()
    return (recs, state_words(st), kept) if keep else (recs, state_words(st))


def lib_stream(B, cam, seq, R, mask=None, host=False, flush_after=(), entry="gyro", profile=False, stamps=None, **kw):
    """streaming driver: seq[k] pushed with R[k] (None: NULL) through the gyro entries (entry = "u8": the existing
    push_frame_u8_device, R unused); flush_after: frame counts after which rebvio_hip_flush is called mid-stream.
    stamps: one per frame in place of k * TS (the driver forms every interval itself).
    (records as words, gyro state after the closing flush[, kernel launches counted by the profiler])"""
    ctx = B.Context(params_for(B, cam, **kw))
    ts = default_stamps(len(seq), stamps)
    npx = cam.width * cam.height
    dev = ctx.upload_frames(seq)
    mdev = ctx.upload_frames(mask[None]) if mask is not None else None
    if profile:
        ctx.profile_reset()
        ctx.profile(True)
    recs = []
    for k in range(len(seq)):
        if entry == "u8":
            out, n = ctx.push_frame_u8_device(dev + k * npx, ts[k])
        elif host:
            out, n = ctx.push_frame_px_gyro(np.ascontiguousarray(seq[k]), B.PX_GRAY8, None if R is None else R[k], ts[k])
        else:
            out, n = ctx.push_frame_px_gyro_device(dev + k * npx, B.PX_GRAY8, None if R is None else R[k], mdev, ts[k])
        if out.status >= 0:
            recs.append(rec(out, n))
        if k + 1 in flush_after:
            recs.extend(rec(o, n) for o, n in ctx.flush())
    recs.extend(rec(o, n) for o, n in ctx.flush())
    st = state_words(ctx.gyro_state())
    launches = None
    if profile:
        launches = {name: calls for name, (_, calls) in ctx.profile_read().items()}
        ctx.profile(False)
    ctx.close()
    return (recs, st, launches) if profile else (recs, st)


# ---- large and wrong rotation priors (tests/test_large_rotations.py holds the oracle to what is written here; the GPU file
# runs the library against it) ------------------------------------------------------------------------------------------
N_TURN = 8             # frames of every stream of these tests (192x144, KW_TRACK)
BAD_PAIR = 3           # the pair 3 -> 4 takes the wrong prior
# w (rad) of the wrong prior rodrigues(w).astype(float32) -> the oracle's status of that pair and its klm_num with the other pairs
# run (a) without a prior, (b) with gyro_rotations(order, 5). Sums in device order. In every row the three pairs behind the bad
# one end with status 0 and at least 1881 (a) / 1906 (b) matches.
WRONG_PRIORS = {
    (0.0, 0.05, 0.0): (0, 1704, 1736),
    (0.02, 0.3, -0.1): (0, 149, 105),
    (0.0, 0.8, 0.0): (0, 72, 61),
    (0.0, np.pi / 2, 0.0): (1, 0, 0),
    (0.3, 1.5, 0.2): (1, 0, 0),
    (0.0, np.pi, 0.0): (1, 0, 0),
    (0.0, 0.0, np.pi / 2): (0, 151, 196),
    (0.0, 0.0, 3.0): (0, 198, 176),
}
ROT90_Y = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], F32)   # the exact fp32 matrices of 90 degrees about y and about x
ROT90_X = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], F32)
# No rotation by +-90 degrees gives a rotated z of -0: the product is summed from +0.0 in double, and +0 + -0 = +0. This matrix
# (no rotation; rotateKeylines takes any) does: z = -2^-100 * (pos_img.x / fm), which for a denormal quotient lies below the
# smallest fp32 denormal and rounds to -0 (to +0 for a negative quotient); every other keyline gets a z around 1e-31.
UNDERFLOW_Z = np.array([[1, 0, 0], [0, 1, 0], [-2.0 ** -100, 0, 0]], F32)
CRAFT_ROTATIONS = {"y90": ROT90_Y, "x90": ROT90_X, "underflow": UNDERFLOW_Z}
# three wrong priors in a row, pairs 2 -> 3, 3 -> 4, 4 -> 5 (the others gyro_rotations(order, 5)): the oracle's status and klm_num
CONSECUTIVE = {2: (0.0, np.pi / 2, 0.0), 3: (0.0, np.pi, 0.0), 4: (0.0, 0.8, 0.0)}
CONSECUTIVE_PAIRS = [(0, 2028), (0, 1995), (1, 0), (1, 0), (0, 217), (0, 1878), (0, 1843)]
# yaw (degrees per frame) of the fast-turn streams -> the oracle's klm_num per pair with the true prior, without a prior (every
# status 0). +6: every pair with the prior has 700 or more, five of seven without it have fewer. No stream of -6, -5 or -4
# degrees meets those bars (with the true prior: -6 below; -5: 214 194 198 [status 1] 315 323 143; -4: 936 326 432 722 439 417 420),
# so the -6 stream stands here with what the oracle gives for it and claims no more than status 0 on every pair.
FAST_TURNS = {
    6.0: ([805, 1052, 1238, 1364, 1327, 1384, 1227], [1335, 348, 603, 625, 594, 498, 422]),
    -6.0: ([704, 495, 541, 428, 217, 352, 273], [1547, 498, 478, 747, 456, 382, 223]),
}
TURN_MIN_KLM = 700
DEPTH_VALUES = (0.0, -1.0, np.inf, np.nan, RHO_MIN, RHO_MAX)   # what the crafted maps put into rho and sigma_rho
CRAFT_SIZES = (1, 63, 64, 65, 256, 257)


def w_id(w):
    return ",".join(f"{v:.3g}" for v in w)


def wrong_prior_rotations(bad, n=N_TURN, stream_id=0, elsewhere="gyro"):
    """gyro_rotations(range(n), 5) - elsewhere = None: no prior - with the prior of pair k -> k + 1 replaced by rodrigues(bad[k])
    for every k of `bad`"""
    R = gyro_rotations(list(range(n)), 5, stream_id) if elsewhere == "gyro" else [None] * n
    for k, w in bad.items():
        R[k + 1] = rodrigues(w).astype(F32)
    return R


_turn_cache = {}


def turn_stream(yaw_deg=None, stream_id=0):
    """(frames [N_TURN, 144, 192], camera, rotations): stream `stream_id` as render_stream gives it (yaw_deg None; rotations
    gyro_rotations(order, 5)), or its scene turning by yaw_deg per frame with the same translation and the true relative
    rotations as priors. Rendered once."""
    key = (yaw_deg, stream_id)
    if key not in _turn_cache:
        from rebvio_amd import synth
        if yaw_deg is None:
            frames, cam = synth.render_stream(192, 144, N_TURN, stream_id=stream_id)
            R = gyro_rotations(list(range(N_TURN)), 5, stream_id)
        else:
            cam = synth.Camera.for_size(192, 144)
            scene = synth.make_scene(stream_id, 1.0)
            scene.yaw_deg = yaw_deg
            frames = np.stack([synth.render_frame(scene, cam, float(t), noise_seed=stream_id * 100003 + t) for t in range(N_TURN)])
            R = [np.eye(3, dtype=F32)]
            for t in range(1, N_TURN):
                Ri, Rj = synth.pose(scene, t - 1)[0], synth.pose(scene, t)[0]
                R.append(((Ri.T @ Rj).T).astype(F32))
        frames = np.ascontiguousarray(frames)
        frames.setflags(write=False)
        _turn_cache[key] = (frames, cam, R)
    return _turn_cache[key]


def craft_rotation_map(kl, n):
    """The first n keylines of a detected map with the inputs that put rotateKeylines (edge_map.cpp:58-71) on its edges under
    ROT90_Y (rotated z = -pos_img.x / fm) and ROT90_X (rotated z = pos_img.y / fm). Keyline i, by i % 8: pos_img.x = +0, -0;
    pos_img.y = +0, -0; pos_img.x, pos_img.y a denormal (so is the quotient by fm); 6, 7 as detected (both signs occur).
    rho = DEPTH_VALUES[i % 7] and sigma_rho = DEPTH_VALUES[(i // 7) % 7], index 6 = as detected."""
    out = kl[:n].copy()
    assert len(out) == n
    i = np.arange(n)
    c = i % 8
    x, y = out["pos_img"][:, 0], out["pos_img"][:, 1]
    x[c == 0], x[c == 1], y[c == 2], y[c == 3] = F32(0.0), F32(-0.0), F32(0.0), F32(-0.0)
    tiny = np.where((i // 8) % 2 == 0, F32(3e-39), F32(-3e-39)).astype(F32)
    x[c == 4] = tiny[c == 4]
    y[c == 5] = tiny[c == 5]
    for f, sel in (("rho", i % 7), ("sigma_rho", (i // 7) % 7)):
        for v in range(6):
            out[f][sel == v] = F32(DEPTH_VALUES[v])
    return out


def rotated_z(kl, R, fm):
    """the third component of rotateKeylines' rotated vector: accumulated in double from 0.0, rounded to fp32 once
    (TooN's makeVector(float, float, 1.0) is a vector of doubles)"""
    with np.errstate(all="ignore"):
        v0 = (kl["pos_img"][:, 0] / F32(fm)).astype(F32).astype(np.float64)
        v1 = (kl["pos_img"][:, 1] / F32(fm)).astype(F32).astype(np.float64)
        R = np.asarray(R, F32).astype(np.float64)
        s = np.zeros(len(kl), np.float64)
        s = s + R[2, 0] * v0
        s = s + R[2, 1] * v1
        s = s + R[2, 2] * 1.0
        return s.astype(F32)


def rotation_classes(kl, R, fm):
    """how many keylines of the crafted map land on each edge of rotateKeylines under R"""
    z = rotated_z(kl, R, fm)
    tiny = np.finfo(F32).tiny
    zero = z == 0
    return dict(plus_zero=int((zero & ~np.signbit(z)).sum()), minus_zero=int((zero & np.signbit(z)).sum()),
                denormal=int(((np.abs(z) > 0) & (np.abs(z) < tiny)).sum()), negative=int((z < 0).sum()),
                **{f"{f}={v}": int((np.isnan(kl[f]) if np.isnan(v) else kl[f] == F32(v)).sum())
                   for f in ("rho", "sigma_rho") for v in DEPTH_VALUES})


def oracle_fusion(orc_mod, po):
    """What the oracle's own glue hands to the second half of a pair (rebvio.cpp:195-203, 225-233): V, P_V, the corrected
    rotation and R0 = SO3::exp of the rotational part of Xgv - the inputs of rebvio_hip_track_pair_finish_async."""
    import ctypes as C
    w = np.array(po.Xgv, F32)[3:].copy()
    R0 = np.zeros(9, F32)
    fp = C.POINTER(C.c_float)
    orc_mod.lib().orc_so3_exp(w.ctypes.data_as(fp), R0.ctypes.data_as(fp))
    return np.array(po.V, F32), np.array(po.P_V, F32), np.array(po.R, F32), R0


# ---- refusals of the on-demand entries: the sentences, the handles, the assertion ---------------------------
DEAD_MAP = "the map's context has been destroyed (rebvio_hip_destroy)"
DEAD_SNAPSHOT = "the snapshot's context has been destroyed (rebvio_hip_destroy)"
DEAD_PLACE_DB = "the place database's context has been destroyed (rebvio_hip_destroy)"


def foreign_snapshot(who):
    return f"{who}: snapshot of another context"


def no_field(who):
    return f"{who}: the map's distance field is not detection's (none was built, or its keylines were uploaded)"


class RefusalScene:
    """The handles a refusal table names. A live context `ctx` with two detected maps (m, m2) and their snapshots (snap, snap2), a
    third map whose keylines were uploaded (up: its field is not detection's) and a place database (db); a second live context
    `other` with a map, its snapshot and a database (fm, fsnap, fdb); the map, snapshot and database of a context that has been
    destroyed (dm, dsnap, ddb). R, t: a pose; nan_R, inf_t: the same with one entry that is not finite."""

    def __init__(self, B, frames, cam, **kw):
        self.B = B
        make = lambda: B.Context(params_for(B, cam, **kw))
        self.ctx, self.other, gone = make(), make(), make()
        self.m, self.m2, self.up = [self.ctx.detect_u8(frames[k], k * TS) for k in range(3)]
        self.up.upload(self.up.keylines())
        self.snap, self.snap2, self.db = self.m.keyframe_snapshot(), self.m2.keyframe_snapshot(), self.ctx.place_db(4)
        self.fm = self.other.detect_u8(frames[0], 0)
        self.fsnap, self.fdb = self.fm.keyframe_snapshot(), self.other.place_db(4)
        self.dm = gone.detect_u8(frames[0], 0)
        self.dsnap, self.ddb = self.dm.keyframe_snapshot(), gone.place_db(4)
        gone.close()
        self.R, self.t = np.eye(3), np.array([0.01, 0.0, 0.0])
        self.nan_R, self.inf_t = np.eye(3), np.array([0.0, 0.0, -np.inf])
        self.nan_R[2, 0] = np.nan
        self.sr = int(self.ctx.p.search_range)

    def close(self):
        for h in (self.snap, self.snap2, self.db, self.fsnap, self.fdb, self.dsnap, self.ddb, self.m, self.m2, self.up, self.fm, self.dm):
            h.release()
        self.ctx.close()
        self.other.close()


def assert_refused(scene, call, rc, text):
    """call(scene) - a binding's method, which raises, or an entry of the library itself, which returns its code - is refused with
    exactly this code and this rebvio_hip_last_error text, and allocates nothing"""
    B = scene.B
    live = B.test_live_resources()
    try:
        got = call(scene)
    except B.HipError as e:
        assert str(e) == f"rebvio_hip error {rc}: {text}", str(e)
    else:
        assert got == rc, got
    assert B.lib().rebvio_hip_last_error().decode() == text
    assert B.test_live_resources() == live


def assert_release_keeps_the_message(B, make):
    """make(context) -> a KfSnapshot or a PlaceDb: released after its context was destroyed (a husk) and while it lives, the handle's
    release leaves rebvio_hip_last_error as an earlier refused call left it - a cleanup path does not replace the reason for it"""
    from rebvio_amd import synth
    _, cam = synth.render_stream(160, 120, 1)
    L = B.lib()
    for destroy_first in (True, False):
        ctx = B.Context(params_for(B, cam, keylines_ref=600, keylines_max=800))
        handle = make(ctx)
        if destroy_first:
            ctx.close()
        assert L.rebvio_hip_map_point_cloud(None, None, None, None, 0, None) == -3     # any refused call: its text is the thread's message now
        text = L.rebvio_hip_last_error().decode()
        assert text and "destroyed" not in text, text
        handle.release()
        assert L.rebvio_hip_last_error().decode() == text
        ctx.close()


# ---- fixtures -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refusal_scene(B):
    """one RefusalScene per test module, on three frames of the 160x120 stream of the keyframe tests"""
    from rebvio_amd import synth
    frames, cam = synth.render_stream(160, 120, 3)
    live = B.test_live_resources()
    scene = RefusalScene(B, frames, cam, keylines_ref=600, keylines_max=800)
    yield scene
    scene.close()
    assert B.test_live_resources() == live


@pytest.fixture(scope="module")
def backend():
    """the binding without a device: the library built if it is missing, nothing run"""
    from rebvio_amd import backend as B
    if not os.path.exists(B.LIB_PATH):
        B.build()
    return B


@pytest.fixture(scope="module")
def B():
    import torch  # noqa: F401  (the bench process has torch's HIP runtime loaded first; do the same here)
    from rebvio_amd import backend
    backend.lib()
    return backend


@pytest.fixture(scope="session")
def ref_mod():
    """oracle/ref_py with oracle/_ref/librebvio_ref.so loaded: the reference's own hot-path sources, compiled. Where the reference
    checkout is present the library is (re)built from it and a failing build fails the test; where it is absent a library that
    travelled with the tree is used as it is. Skips only when there is neither."""
    from oracle import ref_py
    if ref_py.have_reference():
        ref_py.build()
        assert os.path.exists(ref_py.LIB_PATH), "make -C oracle ref left no library"
    elif not os.path.exists(ref_py.LIB_PATH):
        pytest.skip("neither oracle/_ref/librebvio_ref.so nor a reference checkout to build it from")
    ref_py.lib()
    return ref_py


@pytest.fixture(scope="module")
def host_math_tool(tmp_path_factory, host_lib):
    """tests/cpp/host_math_dump.cpp compiled against the host library: run(mode, float32 values) -> its float32 output"""
    exe = str(tmp_path_factory.mktemp("hostmath") / "host_math_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "host_math_dump.cpp"), "-o", exe, "-L", BUILD, "-lrebvio", "-lrebvio_hip",
                    f"-Wl,-rpath,{BUILD}", "-pthread"], check=True)

    def run(mode, values, tmp=os.path.dirname(exe)):
        fi, fo = os.path.join(tmp, "in.f32"), os.path.join(tmp, "out.f32")
        np.asarray(values, np.float32).tofile(fi)
        r = subprocess.run([exe, mode, fi, fo], capture_output=True, text=True)
        assert r.returncode == 0, (mode, r.returncode, r.stderr)
        return np.fromfile(fo, np.float32)
    return run


@pytest.fixture(scope="module")
def host_lib():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "rebvio_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "rebvio_amd", "host")], check=True)
    assert os.path.exists(os.path.join(BUILD, "librebvio.so"))
    return BUILD
