"""The point cloud of a keyframe snapshot without a GPU: the surface (header, binding, exports, the argument checks) and the
library's own per-record statement run on the host (rebvio_hip_test_kf_cloud_host: kfc::record of rebvio_amd/csrc/kf_cloud.hpp, the
source k_kf_cloud_emit compiles) against support.np_cloud applied to the snapshot arrays (tests/kf_cloud_ref.py) - bit for bit:
the definition has no sum and every operation is one rounded fp32 operation, so equality is the derived bound and no tolerance
appears. And the purpose: on the depth fusion's scene a filter on relative depth uncertainty lets more of the fused
keyframe through than of the unfused one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from kf_align_ref import GUARD, oracle_scene
from kf_cloud_ref import DEFAULT, ODD, SIZES, assert_cloud_equal, edge_rows, flt_dict, np_kf_cloud, random_pose, random_snapshot
from kf_fuse_ref import np_kf_fuse, perturbed
from kf_pose_ref import true_motion
from support import CLOUD_DTYPE, F32, ROOT, np_passes
from support import backend  # noqa: F401

ENTRIES = ("rebvio_hip_kf_snapshot_point_cloud", "rebvio_hip_kf_snapshot_point_cloud_async", "rebvio_hip_test_kf_cloud_host")
PURPOSE_SEED = 3            # the draw of tests/test_keyframe_fuse.py's purpose test: the same perturbed keyframe


# ---- the surface ---------------------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "rebvio_hip.h")).read()
    return text, " ".join(re.sub(r"/\*.*?\*/", "", text, flags=re.S).split())


def test_header_declares_the_entries():
    raw, text = _header()
    for decl in ("int rebvio_hip_kf_snapshot_point_cloud(rebvio_hip_kf_snapshot* snap, const rebvio_hip_cloud_filter* filter, "
                 "const rebvio_hip_cloud_pose* pose, rebvio_hip_cloud_point* points_host, int cap, int* count);",
                 "int rebvio_hip_kf_snapshot_point_cloud_async(rebvio_hip_kf_snapshot* snap, const rebvio_hip_cloud_filter* filter, "
                 "const rebvio_hip_cloud_pose* pose, rebvio_hip_cloud** out);",
                 "int rebvio_hip_test_kf_cloud_host(float fm, const float* snap_prs4, const unsigned* snap_matches, int kf_size, "
                 "const rebvio_hip_cloud_filter* filter, const rebvio_hip_cloud_pose* pose, rebvio_hip_cloud_point* points, int cap, "
                 "int* count);"):
        assert decl in text, decl
    assert "#define REBVIO_HIP_ABI_VERSION 3" in text      # additions only
    added = raw[raw.index("Added since"):raw.index("#define REBVIO_HIP_ABI_VERSION")]
    assert "rebvio_hip_kf_snapshot_point_cloud(_async)" in added and "rebvio_hip_test_kf_cloud_host" in added
    assert "gradient_norm = +0.0f" in raw                  # the header says what a snapshot does not keep


def test_binding_and_exports(backend):
    B = backend
    vp, ip, fp, up = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_uint)
    S = B.SIGNATURES
    assert S["rebvio_hip_kf_snapshot_point_cloud"] == (C.c_int, [vp, C.POINTER(B.CloudFilter), C.POINTER(B.CloudPose), vp, C.c_int, ip])
    assert S["rebvio_hip_kf_snapshot_point_cloud_async"] == (C.c_int, [vp, C.POINTER(B.CloudFilter), C.POINTER(B.CloudPose), C.POINTER(vp)])
    assert S["rebvio_hip_test_kf_cloud_host"] == (C.c_int, [C.c_float, fp, up, C.c_int, C.POINTER(B.CloudFilter), C.POINTER(B.CloudPose), vp,
                                                            C.c_int, ip])
    assert callable(B.KfSnapshot.point_cloud) and callable(B.KfSnapshot.point_cloud_async) and callable(B.kf_cloud_host)
    lib = C.CDLL(B.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    # the device entries refuse before they touch a device
    L, n, h = B.lib(), C.c_int(), C.c_void_p()
    err = lambda: L.rebvio_hip_last_error().decode()
    assert L.rebvio_hip_kf_snapshot_point_cloud(None, None, None, None, 0, C.byref(n)) == -3 and "null snapshot" in err()
    assert L.rebvio_hip_kf_snapshot_point_cloud_async(None, None, None, C.byref(h)) == -3 and "null" in err()


# ---- the hook's refusals ---------------------------------------------------------------------------------------------------------------
def test_the_hook_refuses_what_the_entry_refuses(backend):
    B = backend
    prs4, mt = random_snapshot(5, 1)
    nan = float("nan")
    for flt, word in (((2, 0.5, 0.0, 20.0), "rho_min must be > 0"), ((2, 0.5, -1.0, 20.0), "rho_min must be > 0"),
                      ((2, 0.5, 5.0, 4.0), "rho_min > rho_max"), ((2, -0.1, 1e-3, 20.0), "max_rel_sigma must be >= 0"),
                      ((2, nan, 1e-3, 20.0), "NaN"), ((2, 0.5, nan, 20.0), "NaN"), ((2, 0.5, 1e-3, nan), "NaN")):
        with pytest.raises(B.HipError) as e:
            B.kf_cloud_host(100.0, prs4, mt, flt_dict(flt))
        assert "error -3:" in str(e.value) and word in str(e.value), (flt, str(e.value))
    R, t, s = random_pose(1)
    for k in range(13):
        bad = np.concatenate([R.reshape(9), t, [s]]).astype(F32)
        bad[k] = np.nan
        with pytest.raises(B.HipError, match="error -3:.*NaN in the pose"):
            B.kf_cloud_host(100.0, prs4, mt, None, (bad[:9], bad[9:12], bad[12]))
    # null arrays, count and buffer, a negative size and a negative cap: straight at the C entry
    L, n = B.lib(), C.c_int(-1)
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint)
    out = np.full(5, 0xA5A5A5A5, np.uint32).view(np.uint8).repeat(8)
    p, m, o = prs4.ctypes.data_as(fp), mt.ctypes.data_as(up), out.ctypes.data
    hook = L.rebvio_hip_test_kf_cloud_host
    assert hook(100.0, None, m, 5, None, None, o, 5, C.byref(n)) == -3
    assert hook(100.0, p, None, 5, None, None, o, 5, C.byref(n)) == -3
    assert hook(100.0, p, m, 5, None, None, o, 5, None) == -3
    assert hook(100.0, p, m, -1, None, None, o, 5, C.byref(n)) == -3
    assert hook(100.0, p, m, 5, None, None, o, -1, C.byref(n)) == -3
    assert hook(100.0, p, m, 5, None, None, None, 5, C.byref(n)) == -3 and "points buffer" in L.rebvio_hip_last_error().decode()
    assert (out == 0xA5).all() and n.value == -1                     # a refused call wrote nothing
    assert hook(100.0, None, None, 0, None, None, None, 0, C.byref(n)) == 0 and n.value == 0      # an empty snapshot needs no arrays
    # the bounds of the filter themselves are legal
    B.kf_cloud_host(100.0, prs4, mt, flt_dict((0, 0.0, 1e-30, 1e-30)))
    B.kf_cloud_host(100.0, prs4, mt, flt_dict((0xFFFFFFFF, float("inf"), 1.0, float("inf"))))


# ---- by hand ---------------------------------------------------------------------------------------------------------------------------
def test_three_keylines_by_hand(backend):
    """fm 400. Keyline 0: u = 1, v = 0; 1: the principal point; 2: u = -0.5, v = 0.25. Pose: a 90 degree turn about the optical axis
    (x -> y, y -> -x), t = (10, 20, 30), scale 3, so z = 3 / rho: (2, 0, 2) x 3 = (6, 0, 6) -> (0, 6, 6) + t, and so on - every value
    exact in fp32. Keyline 3 fails the filter (matches 1) and leaves no record."""
    fm = 400.0
    prs4 = np.array([[fm, 0.0, 0.5, 0.01], [0.0, 0.0, 4.0, 0.02], [-200.0, 100.0, 0.25, 0.03], [8.0, 8.0, 1.0, 0.01]], F32)
    mt = np.array([3, 2, 7, 1], np.uint32)
    R = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F32)
    c = backend.kf_cloud_host(fm, prs4, mt, None, (R, np.array([10, 20, 30], F32), F32(3.0)))
    assert c.dtype == CLOUD_DTYPE
    assert c["xyz"].tolist() == [[10.0, 26.0, 36.0], [10.0, 20.0, 30.75], [7.0, 14.0, 42.0]]
    assert c["keyline"].tolist() == [0, 1, 2] and c["matches"].tolist() == [3, 2, 7]
    assert c["rho"].tolist() == [0.5, 4.0, 0.25] and c["sigma_rho"].tobytes() == prs4[:3, 3].tobytes()
    assert not c["gradient_norm"].view(np.uint32).any()              # +0.0f: the snapshot keeps no gradient norm
    # no pose: the keyframe's own frame, depth 1 / rho
    c = backend.kf_cloud_host(fm, prs4, mt)
    assert c["xyz"].tolist() == [[2.0, 0.0, 2.0], [0.0, 0.0, 0.25], [-2.0, 1.0, 4.0]]
    assert_cloud_equal(c, np_kf_cloud(prs4, mt, fm), "by hand, no pose")


# ---- the hook against np_cloud ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES + (1000,))
def test_hook_against_np_cloud_bit_for_bit(backend, n):
    for flt in (DEFAULT, ODD):
        prs4, mt = random_snapshot(n, 100 + n, flt)
        for pose, what in ((None, "identity"), (random_pose(n), "random pose")):
            want = np_kf_cloud(prs4, mt, 137.5, flt, pose)
            got, count = backend.kf_cloud_host(137.5, prs4, mt, flt_dict(flt), pose, return_count=True)
            assert count == len(want), (n, what)
            assert_cloud_equal(got, want, f"n {n}, {what}")
            assert np.all(np.diff(got["keyline"]) > 0) and (got["rho"] > 0).all() and np.isfinite(got["xyz"]).all()
        if n >= 64:
            assert 0 < len(want) < n, (n, len(want))
    if n == 1000:                                                     # every planted row is there, and decided as planted
        rows = edge_rows(ODD)
        assert sum(r[5] for r in rows) == 5 and len(rows) == 16
        assert len(want) > 100


def test_every_filter_term_on_its_bound_and_one_ulp_outside(backend):
    for flt in (DEFAULT, ODD, (0, F32(0.1), F32(0.7), F32(0.7))):      # (the last: a range of one value, the rho of the sigma rows)
        rows = edge_rows(flt)
        prs4 = np.array([r[:4] for r in rows], F32)
        mt = np.array([r[4] for r in rows], np.uint32)
        want_idx = [i for i, r in enumerate(rows) if r[5]]
        got = backend.kf_cloud_host(250.0, prs4, mt, flt_dict(flt))
        assert got["keyline"].tolist() == want_idx, (flt, got["keyline"].tolist(), want_idx)
        assert_cloud_equal(got, np_kf_cloud(prs4, mt, 250.0, flt), str(flt))
    # one rounded multiply: 0.1f * 0.7f rounds up to 0.07f, so sigma_rho = 0.07f passes although it exceeds the unrounded product
    prod = F32(0.1) * F32(0.7)
    assert prod == F32(0.07) and float(prod) > float(F32(0.1)) * float(F32(0.7))
    prs4 = np.array([[1, 1, 0.7, np.nextafter(prod, F32(0))], [1, 1, 0.7, prod], [1, 1, 0.7, np.nextafter(prod, F32(1))]], F32)
    got = backend.kf_cloud_host(100.0, prs4, np.full(3, 2, np.uint32), dict(max_rel_sigma=float(F32(0.1))))
    assert got["keyline"].tolist() == [0, 1]


def test_cap_below_count_and_cap_zero(backend):
    B = backend
    prs4, mt = random_snapshot(257, 7)
    full, count = B.kf_cloud_host(90.0, prs4, mt, return_count=True)
    assert count == len(full) > 60
    cap, guard = count // 3, 16
    buf = np.full((cap + guard) * 32, 0xA5, np.uint8)
    n = C.c_int(-1)
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint)
    hook = B.lib().rebvio_hip_test_kf_cloud_host
    assert hook(90.0, prs4.ctypes.data_as(fp), mt.ctypes.data_as(up), 257, None, None, buf.ctypes.data, cap, C.byref(n)) == 0
    assert n.value == count
    assert buf[:cap * 32].tobytes() == full[:cap].tobytes()
    assert (buf[cap * 32:] == 0xA5).all(), "records written beyond cap"
    n = C.c_int(-1)
    assert hook(90.0, prs4.ctypes.data_as(fp), mt.ctypes.data_as(up), 257, None, None, None, 0, C.byref(n)) == 0 and n.value == count
    part, c2 = B.kf_cloud_host(90.0, prs4, mt, cap=1, return_count=True)
    assert c2 == count and part.tobytes() == full[:1].tobytes()
    more, c3 = B.kf_cloud_host(90.0, prs4, mt, cap=count + 9, return_count=True)
    assert c3 == count and more.tobytes() == full.tobytes()


def test_the_per_record_statement_as_a_stand_alone_program(tmp_path):
    """tests/cpp/kf_cloud_host_check.cpp: kfc::record over heap buffers of exactly the needed size, non-finite, denormal and huge
    values in every field, caps of 0, 1 and above the count. Built plainly here; its head says how to build it with sanitizers."""
    import subprocess
    exe = str(tmp_path / "kf_cloud_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rebvio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "kf_cloud_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.stdout[-2000:], r.stderr[-2000:])


# ---- the purpose ---------------------------------------------------------------------------------------------------------------------
def test_a_fused_keyframe_passes_more_keylines_through_a_sigma_filter(backend, orc_mod):
    """The depth fusion's scene: the oracle's 160x120 frame, 1 600 crafted keyframe keylines, rho perturbed within
    sigma_rho, one fusion at the true motion through rebvio_hip_test_kf_fuse_host. The default filter is step 1 of the fusion, and
    a fused keyline stays inside it (rho is clamped to the filter's range and sigma_rho does not grow off the clamps), so the default
    cloud has the same members before and after. With max_rel_sigma at the median sigma_rho / rho of the unfused keylines the default
    filter passes, the fused arrays pass strictly more. Measured: DESIGN.md 5k."""
    B = backend
    scene = oracle_scene(orc_mod)
    R, t = true_motion()
    c = scene["craft"]
    prs4, _ = perturbed(c, PURPOSE_SEED)
    d = (scene["cam"], prs4, c["kf_matches"], c["normals"], scene["pos"], scene["unit"], scene["ids"], scene["dists"])
    assert min(np_kf_fuse(*d, R, t)["guards"].values()) > GUARD
    out, fused4, fused_mt, _ = B.kf_fuse_host(*d[0], scene["search_range"], *d[1:], B.default_kf_fuse_opts(), R, t)
    fm = scene["cam"][0]
    before, after = B.kf_cloud_host(fm, prs4, c["kf_matches"]), B.kf_cloud_host(fm, fused4, fused_mt)
    assert len(prs4) >= 1600 and out.fused > 1000
    assert np.array_equal(before["keyline"], after["keyline"]) and len(before) > 1000
    assert before.tobytes() != after.tobytes()
    kl = np.zeros(len(prs4), np.dtype([("rho", "<f4"), ("sigma_rho", "<f4"), ("matches", "<u4")]))
    kl["rho"], kl["sigma_rho"], kl["matches"] = prs4[:, 2], prs4[:, 3], c["kf_matches"]
    ok = np_passes(kl, *DEFAULT)
    tight = F32(np.median((prs4[ok, 3] / prs4[ok, 2]).astype(F32)))
    flt = dict(max_rel_sigma=float(tight))
    n_before = len(B.kf_cloud_host(fm, prs4, c["kf_matches"], flt))
    n_after = len(B.kf_cloud_host(fm, fused4, fused_mt, flt))
    assert_cloud_equal(B.kf_cloud_host(fm, fused4, fused_mt, flt), np_kf_cloud(fused4, fused_mt, fm, (2, tight, F32(1e-3), F32(20.0))), "fused, tight")
    print(f"keyframe of {len(prs4)} keylines, {out.fused} fused; default filter {len(before)} -> {len(after)}; "
          f"max_rel_sigma {float(tight):.6f} (median of the unfused): {n_before} -> {n_after}")
    assert n_after > n_before
