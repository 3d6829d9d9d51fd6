"""Keyframe snapshot and keyframe-to-current pose without a GPU: the surface (header, binding, exports, struct sizes, defaults, the
argument checks that need no device), the numpy restatement (tests/kf_pose_ref.py) on hand-computed correspondences and against
finite differences, and the library's own solve run on the host (rebvio_hip_test_kf_pose_host: the per-term function and the step of
rebvio_amd/csrc/kf_pose.hpp, the source the kernels compile) against the restatement on the crafted inputs of the GPU tests."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from kf_pose_ref import (DEFAULT_FILTER, craft_arrays, identity_records, np_kf_pose, np_kf_pose_sums, off_guess, pose_err, pose_sums,
                         true_motion, unpack_sums)
from support import F32, KF_MATCH_DTYPE, ROOT, rodrigues
from support import backend  # noqa: F401

ENTRIES = ("rebvio_hip_map_keyframe_snapshot", "rebvio_hip_kf_snapshot_release", "rebvio_hip_kf_snapshot_download",
           "rebvio_hip_default_kf_pose_opts", "rebvio_hip_map_keyframe_pose", "rebvio_hip_test_kf_pose_host")
FM, W, H = 120.0, 160, 120
# |host - numpy| over R and t on the clean crafted cases (item 4 of the GPU file): measured maximum 2.3e-16 (the two differ in the
# summation order, libm's against numpy's sin / cos and the triangular solves, amplified by cond(H) of 20..57); bound = 100 x that.
# It must stay <= 0.1 x the smallest err(np_kf_pose) of these cases (1.05e-9), which test_host_solve_on_clean_data asserts.
HOST_VS_NP = 2.3e-14


# ---- the surface ---------------------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "rebvio_hip.h")).read()
    return " ".join(re.sub(r"/\*.*?\*/", "", text, flags=re.S).split())


def test_header_declares_the_entries_and_structs():
    text = _header()
    for decl in ("int rebvio_hip_map_keyframe_snapshot(rebvio_hip_ctx* ctx, rebvio_hip_map* map, rebvio_hip_kf_snapshot** out);",
                 "void rebvio_hip_kf_snapshot_release(rebvio_hip_kf_snapshot* snap);",
                 "int rebvio_hip_kf_snapshot_download(rebvio_hip_kf_snapshot* snap, float* prs4, unsigned* matches, int cap, int* n);",
                 "void rebvio_hip_default_kf_pose_opts(rebvio_hip_kf_pose_opts* opts);",
                 "int rebvio_hip_map_keyframe_pose(rebvio_hip_map* map, rebvio_hip_kf_snapshot* snap, const rebvio_hip_kf_pose_opts* opts, "
                 "const double R0[9] , const double t0[3] , rebvio_hip_kf_pose* out);"):
        assert decl in text, decl
    m = re.search(r"typedef struct rebvio_hip_kf_pose_opts \{(.*?)\} rebvio_hip_kf_pose_opts;", text)
    assert [f.strip() for f in m.group(1).split(";") if f.strip()] == ["rebvio_hip_cloud_filter kf_filter", "double huber_px", "int max_iter",
                                                                      "int min_used"]
    m = re.search(r"typedef struct rebvio_hip_kf_pose \{(.*?)\} rebvio_hip_kf_pose;", text)
    assert [f.strip() for f in m.group(1).split(";") if f.strip()] == ["double R[9], t[3]", "double H[36], g[6], cost",
                                                                      "int candidates, used, iterations, status"]
    assert "#define REBVIO_HIP_ABI_VERSION 3" in text      # additions only


def test_binding_matches_the_structs(backend):
    B = backend
    vp, ip, dp, fp, up = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint)
    assert B.SIGNATURES["rebvio_hip_map_keyframe_snapshot"] == (C.c_int, [vp, vp, C.POINTER(vp)])
    assert B.SIGNATURES["rebvio_hip_kf_snapshot_release"] == (None, [vp])
    assert B.SIGNATURES["rebvio_hip_kf_snapshot_download"] == (C.c_int, [vp, fp, up, C.c_int, ip])
    assert B.SIGNATURES["rebvio_hip_map_keyframe_pose"] == (C.c_int, [vp, vp, C.POINTER(B.KfPoseOpts), dp, dp, C.POINTER(B.KfPose)])
    # the C layout: a 16-byte filter, a double, two ints; 55 doubles and four ints
    assert C.sizeof(B.KfPoseOpts) == 32 and B.KfPoseOpts.huber_px.offset == 16 and B.KfPoseOpts.max_iter.offset == 24
    assert C.sizeof(B.KfPose) == 55 * 8 + 16
    assert [(n, getattr(B.KfPose, n).offset) for n, _ in B.KfPose._fields_] == [
        ("R", 0), ("t", 72), ("H", 96), ("g", 384), ("cost", 432), ("candidates", 440), ("used", 444), ("iterations", 448), ("status", 452)]
    for method in ("keyframe_snapshot", "keyframe_pose"):
        assert callable(getattr(B.Map, method))
    for method in ("download", "release"):
        assert callable(getattr(B.KfSnapshot, method))


def test_defaults(backend):
    o = backend.default_kf_pose_opts()
    f = backend.default_cloud_filter()
    assert (o.huber_px, o.max_iter, o.min_used) == (2.0, 8, 12)
    assert bytes(o.kf_filter) == bytes(f)
    assert f.min_matches == DEFAULT_FILTER[0]
    assert [F32(f.max_rel_sigma), F32(f.rho_min), F32(f.rho_max)] == [F32(v) for v in DEFAULT_FILTER[1:]]
    o = backend.default_kf_pose_opts(huber_px=3.5, max_iter=0, kf_filter=dict(min_matches=7))
    assert (o.huber_px, o.max_iter, o.min_used, o.kf_filter.min_matches, o.kf_filter.rho_max) == (3.5, 0, 12, 7, 20.0)


def test_library_exports_the_entries_and_refuses_without_a_device(backend):
    B = backend
    lib = C.CDLL(B.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    L = B.lib()
    err = lambda: L.rebvio_hip_last_error().decode()
    h, n, out = C.c_void_p(), C.c_int(), B.KfPose()
    assert L.rebvio_hip_map_keyframe_snapshot(None, None, C.byref(h)) == -3 and "null" in err()
    assert L.rebvio_hip_kf_snapshot_download(None, None, None, 0, C.byref(n)) == -3 and "null" in err()
    assert L.rebvio_hip_map_keyframe_pose(None, None, None, None, None, C.byref(out)) == -3 and "null" in err()
    L.rebvio_hip_kf_snapshot_release(None)


def test_the_host_hook_refuses_what_the_entry_refuses(backend):
    B = backend
    A = craft_arrays(16, 0, FM, W, H)
    rec = identity_records(16)
    args = (FM, A["prs4"], A["kf_matches"], A["cur_pos_img"], A["cur_grad"], rec)
    nan_R = np.eye(3)
    nan_R[1, 2] = np.nan
    for kw, word in ((dict(opts=B.default_kf_pose_opts(huber_px=0.0)), "huber_px"), (dict(opts=B.default_kf_pose_opts(huber_px=float("nan"))), "huber_px"),
                     (dict(opts=B.default_kf_pose_opts(max_iter=-1)), "max_iter"), (dict(opts=B.default_kf_pose_opts(max_iter=33)), "max_iter"),
                     (dict(opts=B.default_kf_pose_opts(min_used=-1)), "min_used"), (dict(opts=B.default_kf_pose_opts(min_used=65537)), "min_used"),
                     (dict(opts=B.default_kf_pose_opts(kf_filter=dict(rho_min=0.0))), "rho_min"),
                     (dict(opts=B.default_kf_pose_opts(kf_filter=dict(rho_min=3.0, rho_max=2.0))), "rho_min > rho_max"),
                     (dict(opts=B.default_kf_pose_opts(kf_filter=dict(max_rel_sigma=-1.0))), "max_rel_sigma"),
                     (dict(opts=B.default_kf_pose_opts(kf_filter=dict(rho_max=float("nan")))), "NaN"),
                     (dict(R0=nan_R), "non-finite"), (dict(t0=[0.0, np.inf, 0.0]), "non-finite")):
        with pytest.raises(B.HipError) as e:
            B.kf_pose_host(*args, **kw)
        assert "error -3:" in str(e.value) and word in str(e.value), (kw, str(e.value))
    for bad in (dict(kf_keyline=16), dict(keyline=-1), dict(keyline=16)):
        r = rec.copy()
        for k, v in bad.items():
            r[k][3] = v
        with pytest.raises(B.HipError, match="error -3:.*indices"):
            B.kf_pose_host(FM, A["prs4"], A["kf_matches"], A["cur_pos_img"], A["cur_grad"], r)
    B.kf_pose_host(*args, opts=B.default_kf_pose_opts(max_iter=32, min_used=65536))      # the bounds themselves are legal


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def hand_case():
    """three correspondences on a camera of fm = 100 at the identity pose, t = (0.1, 0, 0): every figure below follows by hand.
      0: keyframe (10, 20) px, rho 1, seen at (25, 20) with gradient (3, 0):  e = 100 * ((0.1 + 0.1) - 0.25) = -5: outside huber 2
      1: keyframe (0, 0), rho 2, seen at (20, 0) with gradient (0, 4):       n = (0, 1), p = (0.2, 0), e = 0
      2: keyframe (-50, 0), rho 0.5, seen at (-46, 1) with gradient (0, -2):  n = (0, -1), p = (-0.45, 0), e = 100 * (-1)(0 - 0.01) = 1"""
    prs4 = np.array([[10, 20, 1, 0.05], [0, 0, 2, 0.1], [-50, 0, 0.5, 0.02]], F32)
    q = np.array([[25, 20], [20, 0], [-46, 1]], F32)
    g = np.array([[3, 0], [0, 4], [0, -2]], F32)
    return prs4, np.full(3, 3, np.uint32), q, g, identity_records(3)


def test_sums_of_three_hand_computed_correspondences():
    prs4, mt, q, g, rec = hand_case()
    t = np.array([0.1, 0.0, 0.0])
    S, A, used = np_kf_pose_sums(100.0, prs4, mt, q, g, rec, np.eye(3), t, huber=2.0)
    Hm, gv, cost = unpack_sums(S)
    assert used == 3
    # term 0: Y = (0.2, 0.2, 1), c = (100, 0, -20), J = (100, 0, -20, 0.2*-20 - 0, 1*100 + 0.1*20, -0.2*100) = (100, 0, -20, -4, 102, -20),
    #         e = -5, w = 2/5, cost = 2 * (5 - 1) = 8
    # term 1: Y = (0.2, 0, 1), c = (0, 100, 0), J = (0, 200, 0, -100, 0, 0), e = 0, w = 1, cost = 0
    # term 2: Y = (-0.45, 0, 1), c = (0, -100, 0), J = (0, -50, 0, 100, 0, 50), e = 1, w = 1, cost = 0.5
    # (the fp32 quotients 0.1f, 0.2f, ... are 1.5e-8 relative off the decimals used by hand: e is off by 1.5e-7 px, hence the tolerances)
    J = np.array([[100, 0, -20, -4, 102, -20], [0, 200, 0, -100, 0, 0], [0, -50, 0, 100, 0, 50]], np.float64)
    e, w = np.array([-5.0, 0.0, 1.0]), np.array([0.4, 1.0, 1.0])
    assert np.allclose(Hm, (J * w[:, None]).T @ J, rtol=1e-6, atol=1e-3)
    assert np.allclose(gv, (J * w[:, None]).T @ e, rtol=1e-6, atol=1e-3)
    assert cost == pytest.approx(8.5, abs=1e-5)
    assert np.allclose(A[:21], np.abs((J * w[:, None])[:, :, None] * J[:, None, :]).sum(0)[np.triu_indices(6)], rtol=1e-6, atol=1e-3)
    # the skip rules on the same three: a filter that drops term 2 (rho 0.5), a zero gradient on term 1, term 0 behind the camera
    assert np_kf_pose_sums(100.0, prs4, mt, q, g, rec, np.eye(3), t, flt=(2, 0.5, 0.6, 20.0))[2] == 2
    g0 = g.copy()
    g0[1] = 0
    assert np_kf_pose_sums(100.0, prs4, mt, q, g0, rec, np.eye(3), t)[2] == 2
    assert np_kf_pose_sums(100.0, prs4, mt, q, g, rec, np.eye(3), np.array([0.1, 0.0, -1.0]))[2] == 1       # Y.z = 1 - rho: rho 2 and 1 go
    S1, _, _ = np_kf_pose_sums(100.0, prs4, mt, q, g, rec, np.eye(3), t, huber=1e9)
    assert unpack_sums(S1)[2] == pytest.approx(12.5 + 0.5, abs=1e-5)         # plain least squares: e^2 / 2


def test_the_restated_jacobian_against_finite_differences():
    """g = J' W e is the gradient of the cost: central differences of the cost along t and along exp(dw) R, well inside and well outside
    the Huber bound (the cost is C1 across it), on a pose away from the identity"""
    A = craft_arrays(40, 5, FM, W, H, outliers=0.3)
    rec = identity_records(40)
    R, t = off_guess(1)
    args = (FM, A["prs4"], A["kf_matches"], A["cur_pos_img"], A["cur_grad"], rec)
    S, _, used = np_kf_pose_sums(*args, R, t)
    assert used == 40
    _, g, _ = unpack_sums(S)
    h = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        cp = unpack_sums(np_kf_pose_sums(*args, rodrigues(d[3:]) @ R, t + d[:3])[0])[2]
        cm = unpack_sums(np_kf_pose_sums(*args, rodrigues(-d[3:]) @ R, t - d[:3])[0])[2]
        fd = (cp - cm) / (2 * h)
        assert abs(fd - g[k]) <= 1e-6 * max(1.0, abs(g[k])), (k, fd, g[k])


# ---- the library's solve on the host against the restatement -----------------------------------------------------------------------
def _both(backend, A, rec, R0=None, t0=None, **opts):
    args = (FM, A["prs4"], A["kf_matches"], A["cur_pos_img"], A["cur_grad"], rec)
    ref = np_kf_pose(*args, R0, t0, **{("huber" if k == "huber_px" else k): v for k, v in opts.items()})
    got = backend.kf_pose_host(*args, backend.default_kf_pose_opts(**opts), R0, t0)
    return ref, got


def assert_sums_close(got, A, rec, R, t, huber=2.0):
    """every one of the 28 sums within (used + 64) * 2^-52 * sum |term| of the restatement at the same pose"""
    S, absS, used = np_kf_pose_sums(FM, A["prs4"], A["kf_matches"], A["cur_pos_img"], A["cur_grad"], rec, R, t, huber=huber)
    assert got.used == used
    assert (np.abs(pose_sums(got) - S) <= (used + 64) * 2.0 ** -52 * absS).all()


@pytest.mark.parametrize("n", [12, 64, 257, 800])
def test_host_solve_on_clean_data(backend, n):
    A = craft_arrays(n, n, FM, W, H)
    rec = identity_records(n)
    for R0, t0 in ((None, None), off_guess(n)):
        ref, got = _both(backend, A, rec, R0, t0)
        e_np, e_host, d = pose_err(ref["R"], ref["t"]), pose_err(got.R, got.t), pose_err(got.R, got.t, ref["R"], ref["t"])
        print(f"n {n}: err np {e_np:.3g} host {e_host:.3g} |host - np| {d:.3g} cond(H) {np.linalg.cond(ref['H']):.1f}")
        assert ref["status"] == 0 and got.status == 0 and got.iterations == 8 == ref["iterations"]
        assert got.candidates == n and got.used == n == ref["used"]
        assert e_np <= 1e-6 and e_host <= 2 * e_np
        assert HOST_VS_NP <= 0.1 * e_np
        assert d <= HOST_VS_NP
        assert_sums_close(got, A, rec, np.array(got.R), np.array(got.t))     # H, g, cost are those of the RETURNED pose


@pytest.mark.parametrize("n", [800, 257])
def test_host_solve_with_outliers(backend, n):
    A = craft_arrays(n, n, FM, W, H, outliers=0.2)
    rec = identity_records(n)
    ref, got = _both(backend, A, rec)
    ref_ls, got_ls = _both(backend, A, rec, huber_px=1e9)
    e = [pose_err(x["R"], x["t"]) for x in (ref, ref_ls)] + [pose_err(x.R, x.t) for x in (got, got_ls)]
    print(f"n {n}: err np huber {e[0]:.3g} ls {e[1]:.3g}; host huber {e[2]:.3g} ls {e[3]:.3g}")
    assert got.status == 0 == ref["status"] and got_ls.status == 0
    assert e[0] <= 1e-2 and e[2] <= 2 * e[0]
    assert e[1] > 2 * e[0] and e[3] > 2 * e[0]                               # the weights are applied: plain least squares is worse
    assert pose_err(got_ls.R, got_ls.t, ref_ls["R"], ref_ls["t"]) <= 1e-9    # ... and the host follows the restatement there too


def test_host_statuses(backend):
    A = craft_arrays(64, 2, FM, W, H)
    rec = identity_records(64)
    R0, t0 = off_guess(3)
    # used < min_used: status 3, pose = guess, the sums of the guess still returned
    ref, got = _both(backend, A, rec[:11], R0, t0)
    assert ref["status"] == 3 == got.status and got.iterations == 0 and got.used == 11 and got.candidates == 11
    assert np.array_equal(np.array(got.R), R0.reshape(9)) and np.array_equal(np.array(got.t), t0)
    assert_sums_close(got, A, rec[:11], R0, t0)
    assert _both(backend, A, rec[:12], R0, t0)[1].status == 0
    # all gradients parallel (along x: J[1] == 0 in every term, H(1, 1) == 0 exactly): status 2, pose = guess, nothing non-finite
    P = craft_arrays(64, 2, FM, W, H, parallel=True)
    ref, got = _both(backend, P, rec, R0, t0)
    assert ref["status"] == 2 == got.status and got.iterations == 0 and got.used == 64
    assert np.array_equal(np.array(got.R), R0.reshape(9)) and np.array_equal(np.array(got.t), t0)
    assert np.isfinite(np.frombuffer(bytes(got), np.float64, 55)).all() and np.array(got.H).reshape(6, 6)[1, 1] == 0.0
    assert_sums_close(got, P, rec, R0, t0)
    # max_iter 0: the sums at the guess only
    got = backend.kf_pose_host(FM, A["prs4"], A["kf_matches"], A["cur_pos_img"], A["cur_grad"], rec, backend.default_kf_pose_opts(max_iter=0), R0, t0)
    assert got.status == 0 and got.iterations == 0 and np.array_equal(np.array(got.R), R0.reshape(9))
    assert_sums_close(got, A, rec, R0, t0)
    # an empty keyframe: status 3, zero sums
    got = backend.kf_pose_host(FM, np.zeros((0, 4), F32), np.zeros(0, np.uint32), A["cur_pos_img"], A["cur_grad"], np.zeros(0, KF_MATCH_DTYPE))
    assert (got.status, got.candidates, got.used, got.iterations) == (3, 0, 0, 0) and not np.array(got.H).any() and got.R[0] == 1.0
