"""Depth fusion into a keyframe snapshot without a GPU: the surface (header, binding, exports, struct layouts, defaults, the argument
checks), the numpy restatement (tests/kf_fuse_ref.py) on the hand-made 10x8 field of the alignment's tests with one planted keyline
per outcome, de/drho against a central difference, and the library's own per-keyline statement run on the host
(rebvio_hip_test_kf_fuse_host: kfp::fuse_term of rebvio_amd/csrc/kf_pose.hpp, the source the kernel compiles) against the
restatement on an oracle-detected frame with crafted keyframe keylines - bit for bit, since no sum's order could differ - and the
purpose of it all: depths perturbed within their own sigma come closer to the truth.

A comparison between two implementations is valid only while no keyline comes within GUARD of a decision (a cell edge, the min_cos
gate, the innovation gate, info > 0, a clamp) in the restatement; every comparing test asserts that first."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from kf_align_ref import GUARD, oracle_scene
from kf_fuse_ref import COUNTS, INT_MIN, RHO_MAX, RHO_MIN, counts_of, nees, np_kf_fuse, perturbed
from kf_pose_ref import DEFAULT_FILTER, true_motion
from support import F32, ROOT
from support import backend  # noqa: F401

ENTRIES = ("rebvio_hip_default_kf_fuse_opts", "rebvio_hip_kf_snapshot_fuse_depth", "rebvio_hip_test_kf_fuse_host")
PURPOSE_SEED = 3            # the draw of test_fusion_brings_perturbed_depths_closer (chosen on the restatement: gated <= 5 % of associated)


# ---- the surface ---------------------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "rebvio_hip.h")).read()
    return " ".join(re.sub(r"/\*.*?\*/", "", text, flags=re.S).split())


def test_header_declares_the_entries_and_the_structs():
    text = _header()
    for decl in ("void rebvio_hip_default_kf_fuse_opts(rebvio_hip_ctx* ctx , rebvio_hip_kf_fuse_opts* opts);",
                 "int rebvio_hip_kf_snapshot_fuse_depth(rebvio_hip_kf_snapshot* snap, rebvio_hip_map* map, const rebvio_hip_kf_fuse_opts* opts, "
                 "const double R[9], const double t[3], rebvio_hip_kf_fuse* out, int* assoc_host );"):
        assert decl in text, decl
    m = re.search(r"typedef struct rebvio_hip_kf_fuse_opts \{(.*?)\} rebvio_hip_kf_fuse_opts;", text)
    assert [f.strip() for f in m.group(1).split(";") if f.strip()] == ["rebvio_hip_cloud_filter kf_filter", "double min_cos", "double pixel_sigma",
                                                                      "double gate_sigma", "double q_abs", "int max_dist", "int reserved"]
    m = re.search(r"typedef struct rebvio_hip_kf_fuse \{(.*?)\} rebvio_hip_kf_fuse;", text)
    assert [f.strip() for f in m.group(1).split(";") if f.strip()] == ["int " + k for k in COUNTS]
    assert "#define REBVIO_HIP_ABI_VERSION 3" in text      # additions only


def test_binding_matches_the_structs(backend):
    B = backend
    vp, ip, dp, fp, up = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint)
    S = B.SIGNATURES
    assert S["rebvio_hip_default_kf_fuse_opts"] == (None, [vp, C.POINTER(B.KfFuseOpts)])
    assert S["rebvio_hip_kf_snapshot_fuse_depth"] == (C.c_int, [vp, vp, C.POINTER(B.KfFuseOpts), dp, dp, C.POINTER(B.KfFuse), ip])
    assert S["rebvio_hip_test_kf_fuse_host"] == (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, fp, up, fp, C.c_int, fp,
                                                           fp, C.c_int, ip, ip, C.POINTER(B.KfFuseOpts), dp, dp, C.POINTER(B.KfFuse), ip])
    assert C.sizeof(B.KfFuseOpts) == 56 and C.sizeof(B.KfFuse) == 24
    assert [(n, getattr(B.KfFuseOpts, n).offset) for n, _ in B.KfFuseOpts._fields_] == [
        ("kf_filter", 0), ("min_cos", 16), ("pixel_sigma", 24), ("gate_sigma", 32), ("q_abs", 40), ("max_dist", 48), ("reserved", 52)]
    assert [n for n, _ in B.KfFuse._fields_] == list(COUNTS)
    assert callable(B.KfSnapshot.fuse_depth) and callable(B.default_kf_fuse_opts) and callable(B.kf_fuse_host)


def test_defaults(backend):
    o = backend.default_kf_fuse_opts()
    assert (o.min_cos, o.pixel_sigma, o.gate_sigma, o.q_abs, o.max_dist, o.reserved) == (0.9, 1.0, 3.0, 0.0, 40, 0)
    assert bytes(o.kf_filter) == bytes(backend.default_cloud_filter())
    o = backend.default_kf_fuse_opts(gate_sigma=2.0, max_dist=3, kf_filter=dict(min_matches=7))
    assert (o.min_cos, o.gate_sigma, o.max_dist, o.kf_filter.min_matches, o.kf_filter.rho_max) == (0.9, 2.0, 3, 7, 20.0)


def test_library_exports_the_entries_and_refuses_without_a_device(backend):
    B = backend
    lib = C.CDLL(B.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    L = B.lib()
    out = B.KfFuse()
    assert L.rebvio_hip_kf_snapshot_fuse_depth(None, None, None, None, None, C.byref(out), None) == -3
    assert "null" in L.rebvio_hip_last_error().decode()


# ---- the hand-made field -------------------------------------------------------------------------------------------------------------
HC = (100.0, 5.0, 4.0, 8, 10)      # fm, cx, cy, rows, cols
HT = np.array([0.01, 0.0, 0.0])    # R = I, t = HT: u = kx + rho + 5, v = ky + 4 (Y.z = 1)


def hand_case():
    """The field of tests/test_keyframe_align.py's hand case: keyline 0 at (4.25, 4) with unit (1, 0) owns cell (4, 4) at distance 0,
    keyline 1 at (8, 6), unit (0, 1), cell (5, 8) at distance 1, keyline 2 at (2, 2), unit (0.6, 0.8), cell (2, 2); every other cell is
    keyline 0's at distance 5, (6, 6) is empty, (1, 1) belongs to keyline 3 whose unit is zero. With R = I, t = (0.01, 0, 0) a keyframe
    keyline (kx, ky, rho) lands on (kx + rho + 5, ky + 4); against keyline 0: e = kx + rho + 0.75, h = c.x t.x = 100 * 0.01 = 1."""
    pos = np.array([[4.25, 4], [8, 6], [2, 2], [1, 1]], F32)
    unit = np.array([[1, 0], [0, 1], [0.6, 0.8], [0, 0]], F32)
    ids = np.zeros((8, 10), np.int32)
    dists = np.full((8, 10), 5, np.int32)
    for (y, x), (i, d) in {(4, 4): (0, 0), (5, 8): (1, 1), (2, 2): (2, 0), (1, 1): (3, 0)}.items():
        ids[y, x], dists[y, x] = i, d
    ids[6, 6], dists[6, 6] = -1, 0x7FFFFFFF
    return dict(pos=pos, unit=unit, ids=ids.reshape(-1), dists=dists.reshape(-1))


def both(backend, prs4, mt, normals=None, t=HT, flt=DEFAULT_FILTER, **kw):
    """one fusion at R = I, t on the hand field through the restatement and the hook, asserted equal word for word; the restatement"""
    Hc = hand_case()
    prs4, mt = np.array(prs4, F32).reshape(-1, 4), np.array(mt, np.uint32)
    o = dict(min_cos=0.9, max_dist=5, pixel_sigma=1.0, gate_sigma=3.0, q_abs=0.0)
    o.update(kw)
    ref = np_kf_fuse(HC, prs4, mt, normals, Hc["pos"], Hc["unit"], Hc["ids"], Hc["dists"], np.eye(3), t, flt, **o)
    opts = backend.default_kf_fuse_opts(kf_filter=dict(zip(("min_matches", "max_rel_sigma", "rho_min", "rho_max"), flt)), **o)
    got, p2, m2, a2 = backend.kf_fuse_host(*HC, 5, prs4, mt, normals, Hc["pos"], Hc["unit"], Hc["ids"], Hc["dists"], opts, np.eye(3), t)
    assert counts_of(got) == counts_of(ref), (counts_of(got), counts_of(ref))
    assert np.array_equal(a2, ref["assoc"]), (a2, ref["assoc"])
    assert p2.tobytes() == ref["prs4"].tobytes() and np.array_equal(m2, ref["matches"])
    assert got.associated == got.fused + got.gated + got.flat
    return ref


def test_one_planted_keyline_per_outcome(backend):
    # fused: (-2, 0, rho 1, sigma 0.5): e = -0.25, h = 1, v = 0.25, S = 1.25, K = 0.2: rho 1.05, v_n = 0.2, matches 3 -> 4
    r = both(backend, [[-2, 0, 1, 0.5]], [3])
    assert counts_of(r) == (1, 1, 1, 0, 0, 0) and r["assoc"].tolist() == [0] and r["matches"].tolist() == [4]
    assert r["prs4"][0, :2].tolist() == [-2, 0]                                     # pos_img is never written
    assert r["prs4"][0, 2] == pytest.approx(1.05, rel=1e-6) and r["prs4"][0, 3] == pytest.approx(np.sqrt(0.2), rel=1e-6)
    assert r["e"][0] == pytest.approx(-0.25, abs=1e-5) and r["h"][0] == pytest.approx(1.0, rel=1e-6)
    # gated: sigma 0.01: S = 1.0001, e = -0.4 with gate_sigma 0.3: 0.16 > 0.09 * S; inside at gate_sigma 0.5
    g = both(backend, [[-2.15, 0, 1, 0.01]], [3], gate_sigma=0.3)
    assert counts_of(g) == (1, 1, 0, 1, 0, 0) and g["assoc"].tolist() == [-1] and g["matches"].tolist() == [3]
    assert g["prs4"].tobytes() == np.array([[-2.15, 0, 1, 0.01]], F32).tobytes()
    assert counts_of(both(backend, [[-2.15, 0, 1, 0.01]], [3], gate_sigma=0.5)) == (1, 1, 1, 0, 0, 0)
    # against keyline 2 (the id shows in assoc): cell (2, 2) from (-3.4, -2, rho 0.2), u = 1.8, e = 100 * 0.6 * -0.002 = -0.12
    assert both(backend, [[-3.4, -2, 0.2, 0.05]], [3])["assoc"].tolist() == [2]
    assert both(backend, [[-3.4, -2, 0.2, 0.05]], [3], gate_sigma=1e-3)["assoc"].tolist() == [-3]
    # not associated: the filter, an empty cell, max_dist, the owner's zero unit, a NaN sigma_rho (the filter's positive test)
    for row, mt, kw in (([-2, 0, 1, 0.05], 1, {}), ([0, 2, 1, 0.05], 3, {}), ([-3, 1, 1, 0.05], 3, dict(max_dist=4)), ([-5, -3, 1, 0.05], 3, {}),
                        ([-2, 0, 1, np.nan], 3, {})):
        n = both(backend, [row], [mt], **kw)
        assert counts_of(n) == (1, 0, 0, 0, 0, 0) and n["assoc"].tolist() == [INT_MIN], row
        assert n["prs4"].tobytes() == np.array([row], F32).tobytes() and n["matches"].tolist() == [mt]
    # zero sigma_rho with q_abs 0: v = 0, flat; q_abs gives it a variance again
    assert counts_of(both(backend, [[-2, 0, 1, 0.0]], [3])) == (1, 1, 0, 0, 1, 0)
    assert counts_of(both(backend, [[-2, 0, 1, 0.0]], [3], q_abs=0.1)) == (1, 1, 1, 0, 0, 0)
    # the matches word saturates
    assert both(backend, [[-2, 0, 1, 0.5]], [0xFFFFFFFF])["matches"].tolist() == [0xFFFFFFFF]
    # a non-finite update gates: q_abs 1e200 gives v = inf, K = inf / inf = NaN
    n = both(backend, [[-2, 0, 1, 0.5]], [3], q_abs=1e200)
    assert counts_of(n) == (1, 1, 0, 1, 0, 0) and n["assoc"].tolist() == [-1]


def test_clamps(backend):
    wide = (0, 1e9, 1e-3, 20.0)
    # low: rho 0.01, sigma 1 (v = 1, S = 2, K = 0.5), kx = -0.26: e = 0.5 + ... = kx + rho + 0.75 = 0.5: rho_n = 0.01 - 0.25 < RHO_MIN
    lo = both(backend, [[-0.26, 0, 0.01, 1.0]], [3], flt=wide)
    assert counts_of(lo) == (1, 1, 1, 0, 0, 1) and lo["assoc"].tolist() == [0]
    e, K = lo["e"][0], lo["K"][0]
    rho_n = np.float64(F32(0.01)) - K * e
    assert rho_n < RHO_MIN and lo["prs4"][0, 2] == F32(1e-3)
    assert lo["prs4"][0, 3] == F32(np.sqrt((1.0 - K * lo["h"][0]) * 1.0) + (RHO_MIN - rho_n))       # sigma grows by the overshoot
    # high: rho 19.9 lands on u = kx + 24.9 = 4 for kx = -20.9: e = -0.25; sigma 9 (v = 81, K = 81 / 82): rho_n = 19.9 + 0.247
    hi = both(backend, [[-20.9, 0, 19.9, 9.0]], [3], flt=wide)
    assert counts_of(hi) == (1, 1, 1, 0, 0, 1) and hi["prs4"][0, 2] == F32(20.0)
    assert hi["prs4"][0, 3] == F32(np.sqrt((1.0 - hi["K"][0] * hi["h"][0]) * 81.0))                  # sigma as the update left it
    # no clamp in between
    assert counts_of(both(backend, [[-2, 0, 1, 0.5]], [3], flt=wide))[5] == 0


def test_t_zero_is_flat_and_leaves_every_byte(backend):
    prs4 = np.array([[-1, 0, 1, 0.5], [3, 1, 2, 0.1], [-3, -2, 0.5, 0.02], [1, 2, 1, 0.05], [-2, 0, 1, 0.05]], F32)
    mt = np.array([3, 3, 3, 3, 1], np.uint32)
    r = both(backend, prs4, mt, t=np.zeros(3))
    # at t = 0: (kx + 5, ky + 4) = cells (4, 4), (5, 8), (2, 2); the empty cell; the filter
    assert counts_of(r) == (5, 3, 0, 0, 3, 0) and r["assoc"].tolist() == [-1, -2, -3, INT_MIN, INT_MIN]
    assert r["prs4"].tobytes() == prs4.tobytes() and np.array_equal(r["matches"], mt)
    assert (r["h"][:3] == 0).all()


def test_bookkeeping_on_a_mixed_snapshot(backend):
    prs4 = np.array([[-2, 0, 1, 0.5], [-2.15, 0, 1, 0.01], [-2, 0, 1, 0.0], [0, 2, 1, 0.05], [-0.26, 0, 0.01, 1.0], [-3.4, -2, 0.2, 0.05]], F32)
    r = both(backend, prs4, np.full(6, 3, np.uint32), flt=(0, 1e9, 1e-3, 20.0), gate_sigma=0.38)
    assert counts_of(r) == (6, 5, 3, 1, 1, 1) and r["associated"] == r["fused"] + r["gated"] + r["flat"]
    assert r["assoc"].tolist() == [0, -1, -1, INT_MIN, 0, 2]
    # with normals: the gate drops the keyline whose normal crosses its owner's
    nrm = np.array([[1, 0], [1, 0], [1, 0], [1, 0], [0, 1], [0.6, 0.8]], F32)
    assert both(backend, prs4, np.full(6, 3, np.uint32), nrm, flt=(0, 1e9, 1e-3, 20.0), gate_sigma=0.38)["assoc"].tolist() == \
        [0, -1, -1, INT_MIN, INT_MIN, 2]
    assert both(backend, prs4, np.full(6, 3, np.uint32), nrm, flt=(0, 1e9, 1e-3, 20.0), gate_sigma=0.38, min_cos=-1.0)["assoc"].tolist() == \
        [0, -1, -1, INT_MIN, 0, 2]


def test_the_hook_refuses_what_the_entry_refuses(backend):
    B = backend
    Hc = hand_case()
    prs4, mt = np.array([[-2, 0, 1, 0.5]], F32), np.array([3], np.uint32)
    args = (*HC, 5, prs4, mt, None, Hc["pos"], Hc["unit"], Hc["ids"], Hc["dists"])
    nan_R = np.eye(3)
    nan_R[1, 2] = np.nan
    d = lambda **kw: dict(opts=B.default_kf_fuse_opts(max_dist=5, **kw), R=np.eye(3), t=HT)
    for kw, word in ((d(pixel_sigma=0.0), "pixel_sigma"), (d(pixel_sigma=float("nan")), "pixel_sigma"), (d(pixel_sigma=-1.0), "pixel_sigma"),
                     (d(gate_sigma=0.0), "gate_sigma"), (d(gate_sigma=float("nan")), "gate_sigma"), (d(q_abs=-1e-9), "q_abs"),
                     (d(q_abs=float("nan")), "q_abs"), (d(min_cos=-1.01), "min_cos"), (d(min_cos=1.01), "min_cos"), (d(min_cos=float("nan")), "min_cos"),
                     (dict(opts=B.default_kf_fuse_opts(max_dist=-1), R=np.eye(3), t=HT), "max_dist"),
                     (dict(opts=B.default_kf_fuse_opts(max_dist=6), R=np.eye(3), t=HT), "max_dist"), (d(reserved=1), "reserved"),
                     (d(kf_filter=dict(rho_min=0.0)), "rho_min"), (d(kf_filter=dict(rho_min=3.0, rho_max=2.0)), "rho_min > rho_max"),
                     (d(kf_filter=dict(max_rel_sigma=-1.0)), "max_rel_sigma"), (d(kf_filter=dict(rho_max=float("nan"))), "NaN"),
                     (dict(R=nan_R, t=HT), "non-finite"), (dict(R=np.eye(3), t=[0.0, np.inf, 0.0]), "non-finite"),
                     (dict(R=None, t=HT), "null"), (dict(R=np.eye(3), t=None), "null")):
        with pytest.raises(B.HipError) as e:
            B.kf_fuse_host(*args, **kw)
        assert "error -3:" in str(e.value) and word in str(e.value), (kw, str(e.value))
    ids = Hc["ids"].copy()
    ids[17] = 4
    with pytest.raises(B.HipError, match="error -3:.*field id"):
        B.kf_fuse_host(*args[:11], ids, Hc["dists"], R=np.eye(3), t=HT)
    # null arrays, straight at the C entry
    L, out = B.lib(), B.KfFuse()
    fp, up, ip, dp = C.POINTER(C.c_float), C.POINTER(C.c_uint), C.POINTER(C.c_int), C.POINTER(C.c_double)
    R, t = np.eye(3), HT.copy()
    p = dict(prs4=prs4.ctypes.data_as(fp), mt=mt.ctypes.data_as(up), pos=Hc["pos"].ctypes.data_as(fp), unit=Hc["unit"].ctypes.data_as(fp),
             ids=Hc["ids"].ctypes.data_as(ip), dists=Hc["dists"].ctypes.data_as(ip))

    def call(out_p=C.byref(out), **null):
        q = dict(p, **{k: None for k in null})
        return L.rebvio_hip_test_kf_fuse_host(100.0, 5.0, 4.0, 8, 10, 5, q["prs4"], q["mt"], None, 1, q["pos"], q["unit"], 4, q["ids"], q["dists"],
                                              None, R.ctypes.data_as(dp), t.ctypes.data_as(dp), out_p, None)
    for k in p:
        assert call(**{k: 1}) == -3, k
    assert call(out_p=None) == -3
    assert prs4.tobytes() == np.array([[-2, 0, 1, 0.5]], F32).tobytes()          # a refused call wrote nothing
    assert call() == 0 and out.fused == 1                                        # (normals, options and assoc may be null)
    # the bounds themselves are legal
    B.kf_fuse_host(*args, opts=B.default_kf_fuse_opts(max_dist=0, min_cos=-1.0, q_abs=0.0), R=np.eye(3), t=HT)
    B.kf_fuse_host(*args, opts=B.default_kf_fuse_opts(max_dist=5, min_cos=1.0), R=np.eye(3), t=HT)


# ---- the oracle's frame --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(orc_mod):
    return oracle_scene(orc_mod)


def data(scene, prs4=None, normals=True):
    c = scene["craft"]
    return (scene["cam"], c["prs4"] if prs4 is None else prs4, c["kf_matches"], c["normals"] if normals else None, scene["pos"], scene["unit"],
            scene["ids"], scene["dists"])


def host(backend, scene, d, R, t, **opts):
    return backend.kf_fuse_host(*d[0], scene["search_range"], *d[1:], backend.default_kf_fuse_opts(**opts), R, t)


def assert_same(ref, got, what=""):
    """every output word of the hook (or the device) against the restatement's, after its guards"""
    assert min(ref["guards"].values()) > GUARD, (what, ref["guards"])
    out, prs4, mt, assoc = got
    assert counts_of(out) == counts_of(ref), (what, counts_of(out), counts_of(ref))
    assert np.array_equal(assoc, ref["assoc"]), (what, np.flatnonzero(assoc != ref["assoc"])[:8])
    assert np.asarray(prs4, F32).tobytes() == ref["prs4"].tobytes(), (what, np.flatnonzero((np.asarray(prs4) != ref["prs4"]).any(1))[:8])
    assert np.array_equal(mt, ref["matches"]), what
    assert out.associated == out.fused + out.gated + out.flat


def test_h_is_the_derivative_of_e_in_rho(scene):
    """h against (e(rho + d) - e(rho - d)) / 2d at fixed associations. e(rho) = f n . (Z_xy + rho t_xy) / (Z_z + rho t_z) - const is a
    Moebius map of rho: with D = Z_z + rho t_z, e''' = 6 h t_z^2 / D^2, so the central difference is off by d^2 |h| t_z^2 / D^2 (+
    higher orders, a factor (d t_z / D)^2 smaller) and by the rounding of e, 2^-52 |e terms| / d. rho is rounded to fp32 before it is
    used, so the step is a power of two the fp32 rho carries exactly: d = 2^-10 on rho in [0.2, 2.1] (fp32 ulp <= 2^-22). With
    |t_z| = 0.1, D >= 0.9: truncation <= 2^-20 * 0.0124 |h| = 1.2e-8 |h|; rounding <= 2^-52 * 4 * f * 2 / 2^-10 = 1e-10 for f = 100..200.
    Bound: 2e-8 |h| + 1e-9."""
    R, t = true_motion()
    c = scene["craft"]
    ref = np_kf_fuse(*data(scene), R, t)
    sel = np.flatnonzero((ref["assoc"] != INT_MIN) & (c["prs4"][:, 2] > 0.2) & (c["prs4"][:, 2] < 2.1))
    assert len(sel) > 1000
    d = 2.0 ** -10
    es = []
    for sgn in (+1, -1):
        p = np.array(c["prs4"], F32)
        p[:, 2] = (p[:, 2].astype(np.float64) + sgn * d).astype(F32)
        assert ((p[:, 2].astype(np.float64) - c["prs4"][:, 2].astype(np.float64)) == sgn * d)[sel].all()      # the step is exact in fp32
        r = np_kf_fuse(*data(scene, p), R, t, gate_sigma=1e6, flt=(0, 1e9, 1e-3, 20.0))
        own = r["assoc"].astype(np.int64)
        own = np.where(own < 0, -1 - own, own)
        keep = (r["assoc"] != INT_MIN) & (own == np.where(ref["assoc"] < 0, -1 - ref["assoc"].astype(np.int64), ref["assoc"]))
        sel = sel[keep[sel]]                                   # the same owner on both sides of the difference
        es.append(r["e"])
    assert len(sel) > 1000
    fd = (es[0][sel] - es[1][sel]) / (2 * d)
    h = ref["h"][sel]
    err = np.abs(fd - h)
    print(f"h vs central difference over {len(sel)} keylines: max |fd - h| {err.max():.3g}, max |h| {np.abs(h).max():.3g}")
    assert (err <= 2e-8 * np.abs(h) + 1e-9).all(), (err.max(), np.abs(h).max())


@pytest.mark.parametrize("normals", [True, False])
def test_hook_against_the_restatement_bit_for_bit(backend, scene, normals):
    R, t = true_motion()
    prs4, _ = perturbed(scene["craft"], 11)
    for what, kw in (("defaults", {}), ("tight gate, q_abs", dict(gate_sigma=0.8, q_abs=0.02, pixel_sigma=0.5)),
                     ("no gradient test, short reach", dict(min_cos=-1.0, max_dist=1))):
        d = data(scene, prs4, normals)
        ref = np_kf_fuse(*d, R, t, **kw)
        assert_same(ref, host(backend, scene, d, R, t, **kw), what)
        assert ref["fused"] > 500 and (what != "tight gate, q_abs" or ref["gated"] > 0), (what, counts_of(ref))
    # twice: the state carries over
    d = data(scene, prs4, normals)
    once = np_kf_fuse(*d, R, t)
    twice = np_kf_fuse(d[0], once["prs4"], once["matches"], *d[3:], R, t)
    got1 = host(backend, scene, d, R, t)
    got2 = backend.kf_fuse_host(*d[0], scene["search_range"], got1[1], got1[2], *d[3:], backend.default_kf_fuse_opts(), R, t)
    assert_same(twice, got2, "second fusion")
    assert (twice["matches"][twice["assoc"] >= 0] >= 4).all() and twice["prs4"].tobytes() != once["prs4"].tobytes()


def test_inputs_are_left_alone(backend, scene):
    R, t = true_motion()
    d = data(scene)
    before = d[1].tobytes(), d[2].tobytes()
    host(backend, scene, d, R, t)
    np_kf_fuse(*d, R, t)
    assert (d[1].tobytes(), d[2].tobytes()) == before


@pytest.mark.parametrize("side", ["restatement", "hook"])
def test_fusion_brings_perturbed_depths_closer(backend, scene, side):
    """The purpose: crafted depths perturbed by a seeded draw within their own sigma_rho, one fusion at the true motion. Over the fused
    keylines sum (rho - rho_true)^2 / sigma_rho^2 falls strictly, and no fused sigma_rho grows except through a clamp.
    Measured (seed 3, 160x120 oracle frame): see DESIGN.md 5j."""
    R, t = true_motion()
    prs4, rho_true = perturbed(scene["craft"], PURPOSE_SEED)
    d = data(scene, prs4)
    ref = np_kf_fuse(*d, R, t)
    assert min(ref["guards"].values()) > GUARD, ref["guards"]
    assert ref["associated"] > 1000 and ref["gated"] <= 0.05 * ref["associated"], counts_of(ref)
    if side == "restatement":
        after, assoc = ref["prs4"], ref["assoc"]
    else:
        _, after, _, assoc = host(backend, scene, d, R, t)
    fused = assoc >= 0
    low = fused & (after[:, 2] == F32(1e-3))
    assert ((after[:, 3] <= prs4[:, 3]) | low)[fused].all()
    before_sum, after_sum = nees(prs4, rho_true, fused), nees(after, rho_true, fused)
    err = lambda p: float(np.sqrt((((p[:, 2].astype(np.float64) - rho_true) / rho_true) ** 2)[fused].mean()))
    print(f"{side}: counts {counts_of(ref)}; sum of squared normalised errors over {int(fused.sum())} fused keylines {before_sum:.1f} -> {after_sum:.1f}; "
          f"rms relative depth error {err(prs4):.4f} -> {err(after):.4f}; mean sigma_rho / rho "
          f"{float((prs4[:, 3] / prs4[:, 2])[fused].mean()):.4f} -> {float((after[:, 3] / after[:, 2])[fused].mean()):.4f}")
    assert after_sum < before_sum
