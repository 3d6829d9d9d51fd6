"""Point clouds without a GPU: the numpy restatement the GPU tests compare against (tests/support.py: np_cloud),
checked against hand-computed cases, and the PLY writer of rebvio::io round-tripped through tests/cpp/test_point_cloud_ply.cpp."""
import os
import subprocess

import numpy as np
import pytest

from support import BUILD, CLOUD_DTYPE, F32, ROOT, np_cloud, np_passes

OPEN = (0, 1.0, 1e-3, 20.0)


def keylines(rows):
    """(pos_img x, pos_img y, rho, sigma_rho, gradient_norm, matches) per keyline -> the 84-byte records"""
    from rebvio_amd.backend import KEYLINE_DTYPE
    kl = np.zeros(len(rows), KEYLINE_DTYPE)
    for i, (x, y, rho, sig, gn, mt) in enumerate(rows):
        kl["pos_img"][i] = (x, y)
        kl["rho"][i], kl["sigma_rho"][i], kl["gradient_norm"][i], kl["matches"][i] = rho, sig, gn, mt
    return kl


def test_restatement_back_projects_by_hand_computed_cases():
    fm = 400.0
    kl = keylines([(fm, 0.0, 0.5, 0.01, 7.0, 3),          # u = 1, v = 0, z = 1 / 0.5 = 2         -> (2, 0, 2)
                   (0.0, 0.0, 4.0, 0.01, 8.0, 1),         # the principal point at depth 1 / 4     -> (0, 0, 0.25)
                   (-200.0, 100.0, 0.25, 0.01, 9.0, 0)])  # u = -0.5, v = 0.25, z = 4              -> (-2, 1, 4)
    c = np_cloud(kl, fm, OPEN)
    assert c.dtype == CLOUD_DTYPE and c.dtype.itemsize == 32
    assert c["xyz"].tolist() == [[2.0, 0.0, 2.0], [0.0, 0.0, 0.25], [-2.0, 1.0, 4.0]]
    assert c["keyline"].tolist() == [0, 1, 2] and c["matches"].tolist() == [3, 1, 0]
    assert c["rho"].tolist() == [0.5, 4.0, 0.25] and c["gradient_norm"].tolist() == [7.0, 8.0, 9.0]
    # a 90 degree turn about the optical axis (x -> y, y -> -x), a shift and a scale of 3: z = 3 / rho
    R = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F32)
    c = np_cloud(kl, fm, OPEN, (R, np.array([10, 20, 30], F32), F32(3.0)))
    assert c["xyz"].tolist() == [[10.0, 26.0, 36.0], [10.0, 20.0, 30.75], [7.0, 14.0, 42.0]]
    # a 90 degree turn about the y axis (z -> x, x -> -z)
    R = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], F32)
    c = np_cloud(kl, fm, OPEN, (R, np.zeros(3, F32), F32(1.0)))
    assert c["xyz"].tolist() == [[2.0, 0.0, -2.0], [0.25, 0.0, 0.0], [4.0, 1.0, 2.0]]


def test_restatement_filter_terms():
    kl = keylines([(1, 1, 1.0, 0.5, 1, 2), (1, 1, 1.0, np.nextafter(F32(0.5), F32(1)), 1, 2), (1, 1, 1.0, 0.5, 1, 1),
                   (1, 1, 0.0, 0.0, 1, 2), (1, 1, np.nan, 0.0, 1, 2), (1, 1, 1.0, np.nan, 1, 2), (1, 1, np.inf, 0.0, 1, 2),
                   (1, 1, 20.0, 10.0, 1, 2), (1, 1, np.nextafter(F32(20), F32(30)), 1.0, 1, 2), (1, 1, 1e-3, 0.0, 1, 9),
                   (1, 1, np.nextafter(F32(1e-3), F32(0)), 0.0, 1, 9), (1, 1, -1.0, -1.0, 1, 2)])
    assert np_passes(kl, 2, 0.5, 1e-3, 20.0).tolist() == [True, False, False, False, False, False, False, True, False, True, False,
                                                          False]
    # one rounded multiply: the exact product of 0.1f and 0.7f lies below 0.07f and rounds up to it in fp32, so sigma_rho = 0.07f
    # passes although it exceeds the unrounded product; the next float does not
    prod = F32(0.1) * F32(0.7)
    assert prod == F32(0.07) and float(prod) > float(F32(0.1)) * float(F32(0.7))
    kl = keylines([(1, 1, 0.7, np.nextafter(prod, F32(0)), 1, 2), (1, 1, 0.7, prod, 1, 2), (1, 1, 0.7, np.nextafter(prod, F32(1)), 1, 2)])
    assert np_passes(kl, 2, F32(0.1), 1e-3, 20.0).tolist() == [True, True, False]
    c = np_cloud(kl, 100.0, (2, F32(0.1), 1e-3, 20.0))
    assert c["keyline"].tolist() == [0, 1]


def test_ply_writer_round_trips(tmp_path):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "rebvio_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "rebvio_amd", "host")], check=True)
    exe = str(tmp_path / "ply")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_point_cloud_ply.cpp"),
                    "-o", exe, "-L", BUILD, "-lrebvio", "-lrebvio_hip", f"-Wl,-rpath,{BUILD}", "-pthread"], check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    # the file as another reader sees it: numpy on the bytes behind the header
    raw = open(tmp_path / "cloud.ply", "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert b"element vertex 1\n" in head and np.frombuffer(body, "<f4").shape == (4,) and np.frombuffer(body, "<f4")[0] == 1.0
