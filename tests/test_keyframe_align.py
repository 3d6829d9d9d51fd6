"""Snapshot normals and the alignment of a snapshot through a map's distance field without a GPU: the surface (header, binding,
exports, struct layouts, defaults, the argument checks that need no device), the numpy restatement (tests/kf_align_ref.py) on a
hand-computed field and against finite differences, and the library's own per-term lookup and solve run on the host
(rebvio_hip_test_kf_align_host: kfp::align_term and the step of rebvio_amd/csrc/kf_pose.hpp, the source the kernels compile) against
the restatement, on an oracle-detected frame of the 160x120 synthetic stream with keyframe keylines crafted behind a known motion.

A comparison of associations, or of an iterated solve, between the two sides is valid only while no term comes within GUARD of a
cell edge, of the gradient gate or of the Huber switch at any iterate of the restatement: the cases here are chosen so that this
holds, and every comparison asserts it first."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from kf_align_ref import GUARD, OFFSETS, np_kf_align, np_kf_align_sums, offset_guess, oracle_scene
from kf_pose_ref import DEFAULT_FILTER, np_kf_pose_sums, pose_err, pose_sums, true_motion, unpack_sums
from support import F32, KF_MATCH_DTYPE, ROOT, rodrigues
from support import backend  # noqa: F401

ENTRIES = ("rebvio_hip_kf_snapshot_add_normals", "rebvio_hip_kf_snapshot_download_normals", "rebvio_hip_default_kf_align_opts",
           "rebvio_hip_map_keyframe_align", "rebvio_hip_test_kf_align_host")
# |host - numpy| over R and t of the solves of test_host_solve_against_the_restatement and of
# test_host_solve_without_the_gradient_test_follows_the_restatement - measured maximum 3.33e-16 (the two differ in the summation
# order, libm's against numpy's sin / cos and the triangular solves, amplified by cond(H) of 16..17); bound = 100 x that. It must
# stay <= 0.1 x the restatement's own error from the crafted motion, which the first test asserts: 1.14e-9 at the least (at the
# crafted motion itself; 1.64e-6 from the two offsets, where one crafted keyline on a cell edge is associated with its neighbour).
HOST_VS_NP = 3.33e-14


# ---- the surface ---------------------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "rebvio_hip.h")).read()
    return " ".join(re.sub(r"/\*.*?\*/", "", text, flags=re.S).split())


def test_header_declares_the_entries_and_the_struct():
    text = _header()
    for decl in ("int rebvio_hip_kf_snapshot_add_normals(rebvio_hip_kf_snapshot* snap, rebvio_hip_map* map);",
                 "int rebvio_hip_kf_snapshot_download_normals(rebvio_hip_kf_snapshot* snap, float* n2, int cap, int* n);",
                 "void rebvio_hip_default_kf_align_opts(rebvio_hip_ctx* ctx , rebvio_hip_kf_align_opts* opts);",
                 "int rebvio_hip_map_keyframe_align(rebvio_hip_map* map, rebvio_hip_kf_snapshot* snap, const rebvio_hip_kf_align_opts* opts, "
                 "const double R0[9] , const double t0[3] , rebvio_hip_kf_pose* out, int* assoc_host );"):
        assert decl in text, decl
    m = re.search(r"typedef struct rebvio_hip_kf_align_opts \{(.*?)\} rebvio_hip_kf_align_opts;", text)
    assert [f.strip() for f in m.group(1).split(";") if f.strip()] == ["rebvio_hip_cloud_filter kf_filter", "double huber_px", "double min_cos",
                                                                      "int max_dist", "int max_iter, min_used"]
    assert "#define REBVIO_HIP_ABI_VERSION 3" in text      # additions only


def test_binding_matches_the_struct(backend):
    B = backend
    vp, ip, dp, fp, up = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint)
    S = B.SIGNATURES
    assert S["rebvio_hip_kf_snapshot_add_normals"] == (C.c_int, [vp, vp])
    assert S["rebvio_hip_kf_snapshot_download_normals"] == (C.c_int, [vp, fp, C.c_int, ip])
    assert S["rebvio_hip_default_kf_align_opts"] == (None, [vp, C.POINTER(B.KfAlignOpts)])
    assert S["rebvio_hip_map_keyframe_align"] == (C.c_int, [vp, vp, C.POINTER(B.KfAlignOpts), dp, dp, C.POINTER(B.KfPose), ip])
    assert S["rebvio_hip_test_kf_align_host"] == (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, fp, up, fp, C.c_int, fp,
                                                            fp, C.c_int, ip, ip, C.POINTER(B.KfAlignOpts), dp, dp, C.POINTER(B.KfPose), ip])
    # the C layout: a 16-byte filter, two doubles, three ints and four bytes of padding
    assert C.sizeof(B.KfAlignOpts) == 48
    assert [(n, getattr(B.KfAlignOpts, n).offset) for n, _ in B.KfAlignOpts._fields_] == [
        ("kf_filter", 0), ("huber_px", 16), ("min_cos", 24), ("max_dist", 32), ("max_iter", 36), ("min_used", 40)]
    assert callable(B.Map.keyframe_align) and callable(B.KfSnapshot.add_normals) and callable(B.KfSnapshot.normals)
    assert callable(B.default_kf_align_opts) and callable(B.kf_align_host)


def test_defaults(backend):
    o = backend.default_kf_align_opts()
    assert (o.huber_px, o.min_cos, o.max_dist, o.max_iter, o.min_used) == (2.0, 0.9, 40, 8, 12)
    assert bytes(o.kf_filter) == bytes(backend.default_cloud_filter())
    o = backend.default_kf_align_opts(min_cos=-1.0, max_dist=3, kf_filter=dict(min_matches=7))
    assert (o.huber_px, o.min_cos, o.max_dist, o.max_iter, o.kf_filter.min_matches, o.kf_filter.rho_max) == (2.0, -1.0, 3, 8, 7, 20.0)


def test_library_exports_the_entries_and_refuses_without_a_device(backend):
    B = backend
    lib = C.CDLL(B.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    L = B.lib()
    err = lambda: L.rebvio_hip_last_error().decode()
    n, out = C.c_int(), B.KfPose()
    assert L.rebvio_hip_kf_snapshot_add_normals(None, None) == -3 and "null" in err()
    assert L.rebvio_hip_kf_snapshot_download_normals(None, None, 0, C.byref(n)) == -3 and "null" in err()
    assert L.rebvio_hip_map_keyframe_align(None, None, None, None, None, C.byref(out), None) == -3 and "null" in err()


# ---- a hand-computed field ----------------------------------------------------------------------------------------------------------
HC = (100.0, 5.0, 4.0, 8, 10)      # fm, cx, cy, rows, cols
HT = np.array([0.01, 0.0, 0.0])    # the pose of the hand case: R = I, t = HT, so that u = kx + rho + 5 and v = ky + 4


def hand_case():
    """Three keyframe keylines on a 10x8 field, camera fm = 100, (cx, cy) = (5, 4), pose R = I, t = (0.01, 0, 0):
      0: pos_img (-2, 0), rho 1:      p = (-0.01, 0),      (u, v) = (4, 4):     cell (4, 4), owned by keyline 0 at distance 0,
         pos (4.25, 4), unit (1, 0):  q = (-0.75, 0),      e = 100 * (-0.01 + 0.0075) = -0.25
      1: pos_img (1, 1), rho 2:       p = (0.03, 0.01),    (u, v) = (8, 5):     cell (5, 8), owned by keyline 1 at distance 1,
         pos (8, 6), unit (0, 1):     q = (3, 2),          e = 100 * (0.01 - 0.02) = -1: outside huber 0.5
      2: pos_img (-3.2, -2), rho 0.5: p = (-0.027, -0.02), (u, v) = (2.3, 2):   cell (2, 2), owned by keyline 2 at distance 0,
         pos (2, 2), unit (0.6, 0.8): q = (-3, -2),        e = 100 * 0.6 * 0.003 = 0.18
    Every other cell belongs to keyline 0 at distance 5, but (6, 6) is empty and (1, 1) belongs to keyline 3, whose unit is (0, 0)."""
    prs4 = np.array([[-2, 0, 1, 0.05], [1, 1, 2, 0.1], [-3.2, -2, 0.5, 0.02]], F32)
    pos = np.array([[4.25, 4], [8, 6], [2, 2], [1, 1]], F32)
    unit = np.array([[1, 0], [0, 1], [0.6, 0.8], [0, 0]], F32)
    ids = np.zeros((8, 10), np.int32)
    dists = np.full((8, 10), 5, np.int32)
    for (y, x), (i, d) in {(4, 4): (0, 0), (5, 8): (1, 1), (2, 2): (2, 0), (1, 1): (3, 0)}.items():
        ids[y, x], dists[y, x] = i, d
    ids[6, 6], dists[6, 6] = -1, 0x7FFFFFFF
    return dict(prs4=prs4, mt=np.full(3, 3, np.uint32), normals=unit[:3].copy(), pos=pos, unit=unit, ids=ids.reshape(-1), dists=dists.reshape(-1))


def both_sums(backend, Hc, t=HT, normals=True, flt=DEFAULT_FILTER, **kw):
    """one evaluation at R = I, t of the hand case through the restatement and the hook: (sums, used, assoc), asserted equal"""
    nrm = Hc["normals"] if normals else None
    o = dict(huber=0.5, min_cos=0.9, max_dist=5)
    o.update(kw)
    S, _, used, assoc, _ = np_kf_align_sums(HC, Hc["prs4"], Hc["mt"], nrm, Hc["pos"], Hc["unit"], Hc["ids"], Hc["dists"], np.eye(3), t, flt, **o)
    opts = backend.default_kf_align_opts(huber_px=o["huber"], min_cos=o["min_cos"], max_dist=o["max_dist"], max_iter=0, min_used=0,
                                         kf_filter=dict(zip(("min_matches", "max_rel_sigma", "rho_min", "rho_max"), flt)))
    got, a = backend.kf_align_host(*HC, 5, Hc["prs4"], Hc["mt"], nrm, Hc["pos"], Hc["unit"], Hc["ids"], Hc["dists"], opts, np.eye(3), t)
    assert got.status == 0 and got.candidates == len(Hc["prs4"]) and got.used == used and np.array_equal(a, assoc), (a, assoc)
    assert np.allclose(pose_sums(got), S, rtol=1e-13, atol=1e-9)
    return S, used, assoc


def test_sums_of_three_hand_computed_terms(backend):
    S, used, assoc = both_sums(backend, hand_case())
    assert used == 3 and assoc.tolist() == [0, 1, 2]
    Hm, gv, cost = unpack_sums(S)
    # term 0: Y = (-0.01, 0, 1), Z = (-0.02, 0, 1), c = (100, 0, 1),       J = (100, 0, 1, 0, 100.02, 0),                 w = 1
    # term 1: Y = (0.03, 0.01, 1), Z = (0.01, 0.01, 1), c = (0, 100, -1),  J = (0, 200, -2, -100.01, 0.01, 1),            w = 0.5 / 1
    # term 2: Y = (-0.027, -0.02, 1), Z = (-0.032, -0.02, 1), c = (60, 80, 3.22), rho 0.5:
    #         J = (30, 40, 1.61, -0.02 * 3.22 - 80, 60 + 0.032 * 3.22, -0.032 * 80 + 0.02 * 60) = (30, 40, 1.61, -80.0644, 60.10304, -1.36)
    # (the fp32 quotients and the fp32 unit (0.6, 0.8) are ~3e-8 relative off the decimals used by hand: hence the tolerances)
    J = np.array([[100, 0, 1, 0, 100.02, 0], [0, 200, -2, -100.01, 0.01, 1], [30, 40, 1.61, -80.0644, 60.10304, -1.36]], np.float64)
    e, w = np.array([-0.25, -1.0, 0.18]), np.array([1.0, 0.5, 1.0])
    assert np.allclose(Hm, (J * w[:, None]).T @ J, rtol=1e-5, atol=1e-3)
    assert np.allclose(gv, (J * w[:, None]).T @ e, rtol=1e-5, atol=2e-3)
    assert cost == pytest.approx(0.25 ** 2 / 2 + 0.5 * (1.0 - 0.25) + 0.18 ** 2 / 2, abs=1e-5)


def planted(Hc, kx, ky, rho=1.0, matches=3, normal=(1.0, 0.0)):
    """the hand case with a fourth keyframe keyline; at the hand pose it projects to (u, v) = (kx + rho + 5, ky + 4)"""
    P = dict(Hc)
    P["prs4"] = np.concatenate([Hc["prs4"], np.array([[kx, ky, rho, 0.05 * rho]], F32)])
    P["mt"] = np.append(Hc["mt"], np.uint32(matches))
    P["normals"] = np.concatenate([Hc["normals"], np.array([normal], F32)])
    return P


def test_every_skip_rule_drops_exactly_its_keyline(backend):
    Hc = hand_case()
    kept, dropped = [0, 1, 2, 0], [0, 1, 2, -1]

    def run(P, **kw):
        return both_sums(backend, P, **kw)[2].tolist()

    on44 = (-2.0, 0.0)                                        # lands on cell (4, 4) like keyline 0
    assert run(planted(Hc, *on44)) == kept                    # the planted keyline as such is used
    assert run(planted(Hc, *on44, matches=1)) == dropped      # 1. the filter (min_matches 2)
    assert run(planted(Hc, *on44), flt=(2, 0.5, 1e-3, 1.5)) == [0, -1, 2, 0]      # ... and rho_max on keyline 1's rho 2
    # 2. Y.z = 1 - 0.06 * 19 < 0; the other three stay in their cells: (3.94, 4), (8.41, 5.14), (2.22, 1.94)
    tz = np.array([0.01, 0.0, -0.06])
    assert run(planted(Hc, *on44, rho=19.0), t=tz) == dropped
    assert run(planted(Hc, *on44, rho=1.0), t=tz) == kept
    # 3. the image bounds x in 1..8, y in 1..6: just outside on each side (the cells there are not empty), and the rim itself
    for kx, ky, want in ((-5.7, 0.0, -1), (3.0, 0.0, -1), (0.0, -3.6, -1), (0.0, 2.7, -1), (-5.0, 0.4, 0), (2.0, 0.0, 0), (0.0, -3.0, 0),
                         (1.3, 2.0, 0)):
        assert run(planted(Hc, kx, ky, normal=(0.0, 0.0))) == [0, 1, 2, want], (kx, ky)
    # 4. an empty cell, (6, 6); a cell at distance 5 against max_dist 4 and 5
    assert run(planted(Hc, 0.0, 2.0)) == dropped
    assert run(planted(Hc, -3.0, 1.0), max_dist=4) == dropped
    assert run(planted(Hc, -3.0, 1.0), max_dist=5) == kept
    assert run(planted(Hc, -3.0, 1.0), max_dist=0) == [0, -1, 2, -1]          # keyline 1's cell is at distance 1
    # 5. the gate: a normal across the owner's (cos 0), one at cos 0.8 against min_cos 0.9 and 0.7, the gate switched off, no normals
    assert run(planted(Hc, *on44, normal=(0.0, 1.0))) == dropped
    assert run(planted(Hc, *on44, normal=(0.8, 0.6))) == dropped
    assert run(planted(Hc, *on44, normal=(0.8, 0.6)), min_cos=0.7) == kept
    assert run(planted(Hc, *on44, normal=(0.0, 1.0)), min_cos=-1.0) == kept
    assert run(planted(Hc, *on44, normal=(0.0, 1.0)), normals=False) == kept
    assert run(planted(Hc, *on44, normal=(-1.0, 0.0))) == dropped             # opposite polarity
    #    a zero normal: no gate, the term is kept
    assert run(planted(Hc, *on44, normal=(0.0, 0.0))) == kept
    # 6. the owner's unit is zero (keyline 3 on cell (1, 1)): kfp::term's own skip, with and without a normal to gate
    assert run(planted(Hc, -5.0, -3.0)) == dropped
    assert run(planted(Hc, -5.0, -3.0, normal=(0.0, 0.0))) == dropped


def test_the_host_hook_refuses_what_the_entry_refuses(backend):
    B = backend
    Hc = hand_case()
    args = (*HC, 5, Hc["prs4"], Hc["mt"], Hc["normals"], Hc["pos"], Hc["unit"], Hc["ids"], Hc["dists"])
    nan_R = np.eye(3)
    nan_R[1, 2] = np.nan
    d = lambda **kw: dict(opts=B.default_kf_align_opts(max_dist=5, **kw))
    for kw, word in ((d(huber_px=0.0), "huber_px"), (d(huber_px=float("nan")), "huber_px"), (d(max_iter=-1), "max_iter"), (d(max_iter=33), "max_iter"),
                     (d(min_used=-1), "min_used"), (d(min_used=65537), "min_used"), (d(min_cos=-1.01), "min_cos"), (d(min_cos=1.01), "min_cos"),
                     (d(min_cos=float("nan")), "min_cos"), (dict(opts=B.default_kf_align_opts(max_dist=-1)), "max_dist"),
                     (dict(opts=B.default_kf_align_opts(max_dist=6)), "max_dist"),
                     (d(kf_filter=dict(rho_min=0.0)), "rho_min"), (d(kf_filter=dict(rho_min=3.0, rho_max=2.0)), "rho_min > rho_max"),
                     (d(kf_filter=dict(max_rel_sigma=-1.0)), "max_rel_sigma"), (d(kf_filter=dict(rho_max=float("nan"))), "NaN"),
                     (dict(R0=nan_R), "non-finite"), (dict(t0=[0.0, np.inf, 0.0]), "non-finite")):
        with pytest.raises(B.HipError) as e:
            B.kf_align_host(*args, **kw)
        assert "error -3:" in str(e.value) and word in str(e.value), (kw, str(e.value))
    ids = Hc["ids"].copy()
    ids[17] = 4                                                # four keylines: ids 0..3
    with pytest.raises(B.HipError, match="error -3:.*field id"):
        B.kf_align_host(*args[:11], ids, Hc["dists"])
    # null arrays, straight at the C entry
    L, out = B.lib(), B.KfPose()
    fp, up, ip = C.POINTER(C.c_float), C.POINTER(C.c_uint), C.POINTER(C.c_int)
    p = dict(prs4=Hc["prs4"].ctypes.data_as(fp), mt=Hc["mt"].ctypes.data_as(up), pos=Hc["pos"].ctypes.data_as(fp), unit=Hc["unit"].ctypes.data_as(fp),
             ids=Hc["ids"].ctypes.data_as(ip), dists=Hc["dists"].ctypes.data_as(ip))

    def call(out_p=C.byref(out), **null):
        q = dict(p, **{k: None for k in null})
        return L.rebvio_hip_test_kf_align_host(100.0, 5.0, 4.0, 8, 10, 5, q["prs4"], q["mt"], None, 3, q["pos"], q["unit"], 4, q["ids"], q["dists"],
                                               None, None, None, out_p, None)
    assert call() == 0 and out.used == 3                       # (normals, options, guess and assoc may be null)
    for k in p:
        assert call(**{k: 1}) == -3, k
    assert call(out_p=None) == -3
    B.kf_align_host(*args, opts=B.default_kf_align_opts(max_dist=5, max_iter=32, min_used=65536, min_cos=1.0))     # the bounds themselves are legal
    B.kf_align_host(*args, opts=B.default_kf_align_opts(max_dist=0, min_cos=-1.0))


# ---- the oracle's frame --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(orc_mod):
    return oracle_scene(orc_mod)


def data(scene, normals=True, n=None):
    c = scene["craft"]
    return (scene["cam"], c["prs4"][:n], c["kf_matches"][:n], c["normals"][:n] if normals else None, scene["pos"], scene["unit"], scene["ids"],
            scene["dists"])


def host(backend, scene, d, R0, t0, **opts):
    cam = d[0]
    return backend.kf_align_host(*cam, scene["search_range"], *d[1:], backend.default_kf_align_opts(**opts), R0, t0)


def test_the_scene_is_what_the_cases_assume(scene):
    c = scene["craft"]
    assert len(scene["kl"]) == 1601 and len(c["prs4"]) >= 1500 and (scene["ids"] >= 0).mean() > 0.9
    # crafted keyframe keylines project onto their owners' cells at the crafted motion: all but a few that sit on a cell edge
    R, t = true_motion()
    _, _, used, assoc, g = np_kf_align_sums(*data(scene), R, t)
    assert used == len(c["prs4"]) and (assoc == c["owner"]).mean() > 0.99 and min(g.values()) > GUARD


def test_the_restated_jacobian_against_finite_differences(scene):
    """g = J' W e is the gradient of the cost at FIXED associations: central differences of the cost of the correspondences the
    evaluation chose, along t and along exp(dw) R, at a pose off the crafted motion"""
    d = data(scene)
    cam = d[0]
    R, t = offset_guess(*OFFSETS[0])
    S, _, used, assoc, _ = np_kf_align_sums(*d, R, t)
    assert used > 500
    _, g, _ = unpack_sums(S)
    rec = np.zeros(used, KF_MATCH_DTYPE)
    rec["kf_keyline"], rec["keyline"] = np.flatnonzero(assoc >= 0), assoc[assoc >= 0]
    q = (scene["pos"] - np.array([cam[1], cam[2]], F32)).astype(F32)
    fixed = (cam[0], d[1], d[2], q, scene["unit"], rec)
    S_fixed, _, used_fixed = np_kf_pose_sums(*fixed, R, t)
    assert used_fixed == used and np.array_equal(S_fixed, S)       # the same terms, through the pose entry's restatement
    h = 1e-6
    for k in range(6):
        dv = np.zeros(6)
        dv[k] = h
        cp = unpack_sums(np_kf_pose_sums(*fixed, rodrigues(dv[3:]) @ R, t + dv[:3])[0])[2]
        cm = unpack_sums(np_kf_pose_sums(*fixed, rodrigues(-dv[3:]) @ R, t - dv[:3])[0])[2]
        fd = (cp - cm) / (2 * h)
        assert abs(fd - g[k]) <= 1e-6 * max(1.0, abs(g[k])), (k, fd, g[k])


def assert_evaluation(backend, scene, d, R, t, what, **opts):
    """one evaluation (max_iter 0) on both sides at (R, t): guards, assoc element for element, the 28 sums within the bound"""
    kw = {("huber" if k == "huber_px" else k): v for k, v in opts.items()}
    S, absS, used, assoc, g = np_kf_align_sums(*d, R, t, **kw)
    assert min(g.values()) > GUARD, (what, g)
    got, a = host(backend, scene, d, R, t, max_iter=0, **opts)
    assert np.array_equal(a, assoc), (what, np.flatnonzero(a != assoc)[:8])
    assert got.used == used and got.candidates == len(d[1]) and got.iterations == 0
    diff = np.abs(pose_sums(got) - S)
    bound = (used + 64) * 2.0 ** -52 * absS
    assert (diff <= bound).all(), (what, np.flatnonzero(diff > bound))
    return used


@pytest.mark.parametrize("normals", [True, False])
def test_host_sums_and_associations_against_the_restatement(backend, scene, normals):
    d = data(scene, normals)
    R, t = true_motion()
    assert assert_evaluation(backend, scene, d, R, t, "truth") == len(d[1])
    for k, (rot, tr) in enumerate(OFFSETS + ((0.05, 0.2),)):
        used = assert_evaluation(backend, scene, d, *offset_guess(rot, tr), f"offset {k}")
        assert 12 <= used < len(d[1])
    rng = np.random.default_rng(7)
    used = assert_evaluation(backend, scene, d, rodrigues(rng.uniform(-0.1, 0.1, 3)), rng.uniform(-0.2, 0.2, 3), "random", huber_px=0.7, min_cos=0.5,
                             max_dist=6)
    assert used > 0


@pytest.mark.parametrize("rot,tr", [(0.0, 0.0)] + list(OFFSETS))
def test_host_solve_against_the_restatement(backend, scene, rot, tr):
    d = data(scene)
    R0, t0 = offset_guess(rot, tr)
    ref = np_kf_align(*d, R0, t0)
    assert ref["guard"] > GUARD, ref["guard"]
    got, assoc = host(backend, scene, d, R0, t0)
    e_np, e_host, dd = pose_err(ref["R"], ref["t"]), pose_err(got.R, got.t), pose_err(got.R, got.t, ref["R"], ref["t"])
    print(f"offset ({rot}, {tr}): err np {e_np:.3g} host {e_host:.3g} |host - np| {dd:.3g} used {got.used} cond(H) {np.linalg.cond(ref['H']):.1f} "
          f"guard {ref['guard']:.3g}")
    assert ref["status"] == 0 == got.status and got.iterations == 8 == ref["iterations"]
    assert got.used == ref["used"] and got.candidates == len(d[1]) and np.array_equal(assoc, ref["assoc"])
    assert e_np <= 1e-5                                         # the restatement converges from this offset (with the gradient test)
    assert HOST_VS_NP <= 0.1 * e_np
    assert dd <= HOST_VS_NP
    # H, g, cost and assoc are those of the RETURNED pose
    S, absS, used, a2, _ = np_kf_align_sums(*d, np.array(got.R), np.array(got.t))
    assert used == got.used and np.array_equal(a2, assoc)
    assert (np.abs(pose_sums(got) - S) <= (used + 64) * 2.0 ** -52 * absS).all()


@pytest.mark.parametrize("rot,tr", list(OFFSETS))
def test_host_solve_without_the_gradient_test_follows_the_restatement(backend, scene, rot, tr):
    """min_cos = -1: crossing edges steal associations and the solve need not converge - only host == restatement is asked"""
    d = data(scene)
    R0, t0 = offset_guess(rot, tr)
    ref = np_kf_align(*d, R0, t0, min_cos=-1.0)
    assert ref["guard"] > GUARD, ref["guard"]
    got, assoc = host(backend, scene, d, R0, t0, min_cos=-1.0)
    none, assoc_none = host(backend, scene, data(scene, normals=False), R0, t0)
    assert bytes(none) == bytes(got) and np.array_equal(assoc_none, assoc)      # no normals at all: the same thing
    dd = pose_err(got.R, got.t, ref["R"], ref["t"])
    print(f"offset ({rot}, {tr}) without the gate: err np {pose_err(ref['R'], ref['t']):.3g} host {pose_err(got.R, got.t):.3g} "
          f"|host - np| {dd:.3g} used {got.used} cond(H) {np.linalg.cond(ref['H']):.1f}")
    assert got.status == ref["status"] and got.iterations == ref["iterations"] and got.used == ref["used"]
    assert np.array_equal(assoc, ref["assoc"])
    assert dd <= HOST_VS_NP


def test_host_statuses(backend, scene):
    R0, t0 = offset_guess(*OFFSETS[0])
    # used < min_used at the first evaluation: status 3, the pose stays the guess, the sums of the guess are returned
    d = data(scene, n=11)
    got, assoc = host(backend, scene, d, R0, t0)
    assert got.status == 3 and got.iterations == 0 and got.candidates == 11 and got.used == (assoc >= 0).sum() <= 11
    assert np.array_equal(np.array(got.R), R0.reshape(9)) and np.array_equal(np.array(got.t), t0)
    S, absS, used, a2, _ = np_kf_align_sums(*d, R0, t0)
    assert used == got.used and np.array_equal(a2, assoc) and (np.abs(pose_sums(got) - S) <= (used + 64) * 2.0 ** -52 * absS).all()
    assert np_kf_align(*d, R0, t0)["status"] == 3
    # every unit along x: J[1] == 0 in every term, H(1, 1) == 0 exactly: status 2, nothing non-finite
    d = list(data(scene, normals=False))
    d[5] = np.tile(np.array([[1.0, 0.0]], F32), (len(scene["unit"]), 1))
    got, _ = host(backend, scene, d, R0, t0)
    ref = np_kf_align(*d, R0, t0)
    assert ref["status"] == 2 == got.status and got.iterations == 0 and got.used == ref["used"] > 12
    assert np.array_equal(np.array(got.R), R0.reshape(9)) and np.isfinite(np.frombuffer(bytes(got), np.float64, 55)).all()
    assert np.array(got.H).reshape(6, 6)[1, 1] == 0.0
    # an empty snapshot: status 3, the guess, zero sums
    got, assoc = host(backend, scene, data(scene, n=0), R0, t0)
    assert (got.status, got.candidates, got.used, got.iterations) == (3, 0, 0, 0) and not np.array(got.H).any() and len(assoc) == 0
    assert np.array_equal(np.array(got.R), R0.reshape(9))
