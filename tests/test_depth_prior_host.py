"""The depth prior above the C-ABI: the per-keyline statements as a stand-alone program under sanitizers (CPU), and on the GPU
rebvio::EdgeMap::fuseDepthImage, rebvio::Rebvio::depthImageCallback (tests/cpp/test_depth_prior.cpp says what it checks) and
`rebvio_replay --depth`."""
import os
import subprocess

import numpy as np
import pytest

from support import host_lib  # noqa: F401
from support import ROOT

N, W, H = 12, 160, 120


def test_the_per_keyline_statements_as_a_stand_alone_program_under_sanitizers(tmp_path):
    """tests/cpp/depth_prior_host_check.cpp over rebvio_amd/csrc/depth_prior.hpp alone, built with AddressSanitizer and
    UndefinedBehaviorSanitizer: depth images in heap buffers of exactly the bytes that may be read, keylines at hostile positions,
    every outcome reached. A program of its own on the CPU; nothing of it is loaded into this process."""
    exe = str(tmp_path / "depth_prior_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rebvio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "depth_prior_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


@pytest.fixture(scope="module")
def stream_files(tmp_path_factory):
    from rebvio_amd import synth
    d = tmp_path_factory.mktemp("depthprior")
    frames, cam = synth.render_stream(W, H, N)
    depth = np.rint(synth.render_stream_depth(W, H, N).astype(np.float64) * 1000.0).astype("<u2")
    ts, gyro, acc = synth.imu_samples(synth.make_scene(0), N, noise_seed=1)
    fp, dp, ip = d / "frames.u8", d / "depth.u16", d / "imu.bin"
    frames.tofile(fp)
    depth.tofile(dp)
    rec = np.zeros(len(ts), dtype=[("ts", "<i8"), ("gyro", "<f4", 3), ("acc", "<f4", 3)])
    rec["ts"], rec["gyro"], rec["acc"] = ts, gyro, acc
    rec.tofile(ip)
    return d, fp, dp, ip, cam


@pytest.mark.gpu
def test_classes_and_callbacks(host_lib, stream_files):
    d, fp, dp, ip, cam = stream_files
    exe = str(d / "depth_prior")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_depth_prior.cpp"), "-o", exe, "-L", host_lib, "-lrebvio", "-lrebvio_hip",
                    f"-Wl,-rpath,{host_lib}", "-pthread"], check=True)
    r = subprocess.run([exe, str(fp), str(dp), str(W), str(H), str(N), repr(cam.fm), repr(cam.cx), repr(cam.cy), "600", "800", str(ip), "50"],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-6000:], r.stderr[-2000:])


@pytest.mark.gpu
def test_replay_reads_a_raw_depth_file(host_lib, stream_files):
    """--depth FILE [--depth-unit U]: every frame's image is fused (none dropped); the plain run is what it is run after
    run; --depth-unit is taken (a file of half the counts at 0.002 m per count fuses every frame too)"""
    d, fp, dp, ip, cam = stream_files
    odo0, odo0b, odo1, odo2 = d / "odometry0.txt", d / "odometry0b.txt", d / "odometry1.txt", d / "odometry2.txt"
    base = [os.path.join(host_lib, "rebvio_replay"), "--raw", str(fp), "--size", str(W), str(H), "--imu", str(ip), "--camera", repr(cam.fm),
            repr(cam.cx), repr(cam.cy), "--keylines", "600", "800", "--min-matches", "50"]
    for out in (odo0, odo0b):
        r0 = subprocess.run(base + ["--out", str(out)], capture_output=True, text=True, timeout=300)
        assert r0.returncode == 0 and "depth_images" not in r0.stderr, (r0.stdout, r0.stderr[-2000:])
    assert open(odo0).read() == open(odo0b).read()
    r = subprocess.run(base + ["--out", str(odo1), "--depth", str(dp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert f"depth_images={N} depth_fused_frames={N} " in r.stderr and "depth_dropped=0" in r.stderr, r.stderr[-2000:]
    half = d / "depth_half.u16"
    (np.fromfile(dp, "<u2") // 2).astype("<u2").tofile(half)
    r = subprocess.run(base + ["--out", str(odo2), "--depth", str(half), "--depth-unit", "0.002"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"depth_fused_frames={N} " in r.stderr, (r.stdout, r.stderr[-2000:])
    for bad in (["--depth"], ["--depth", str(dp), "--depth-unit", "0"], ["--depth", str(d / "missing.u16")]):
        b = subprocess.run(base + ["--out", str(odo2)] + bad, capture_output=True, text=True, timeout=60)
        assert b.returncode in (1, 2), (bad, b.returncode, b.stderr[-500:])
