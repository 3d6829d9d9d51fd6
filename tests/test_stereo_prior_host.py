"""The stereo prior above the C-ABI: the statements as a stand-alone program under sanitizers (CPU), and on the GPU
rebvio::EdgeMap::fuseStereo, rebvio::Rebvio::rightImageCallback (tests/cpp/test_stereo_prior.cpp says what it checks) and
`rebvio_replay --right`."""
import os
import subprocess

import numpy as np
import pytest

from support import host_lib  # noqa: F401
from support import ROOT

N, W, H, BASELINE = 12, 160, 120, 0.2


def test_the_statements_as_a_stand_alone_program_under_sanitizers(tmp_path):
    """tests/cpp/stereo_prior_host_check.cpp over rebvio_amd/csrc/stereo_prior.hpp alone, built with AddressSanitizer and
    UndefinedBehaviorSanitizer: the right map's mask and keyline table in heap buffers of exactly the bytes that may be read, left
    keylines at hostile positions, the window walked cell by cell and as sixteen lanes, every outcome reached. A program of its
    own on the CPU; nothing of it is loaded into this process."""
    exe = str(tmp_path / "stereo_prior_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rebvio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "stereo_prior_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


@pytest.fixture(scope="module")
def stream_files(tmp_path_factory):
    from rebvio_amd import synth
    d = tmp_path_factory.mktemp("stereoprior")
    left, right, cam = synth.render_stereo_stream(W, H, N, BASELINE)
    scene = synth.make_scene(0)
    ts, gyro, acc = synth.imu_samples(scene, N, noise_seed=1)
    lp, rp, ip = d / "left.u8", d / "right.u8", d / "imu.bin"
    left.tofile(lp)
    right.tofile(rp)
    rec = np.zeros(len(ts), dtype=[("ts", "<i8"), ("gyro", "<f4", 3), ("acc", "<f4", 3)])
    rec["ts"], rec["gyro"], rec["acc"] = ts, gyro, acc
    rec.tofile(ip)
    return d, lp, rp, ip, cam, scene


@pytest.mark.gpu
def test_classes_and_callbacks(host_lib, stream_files):
    d, lp, rp, ip, cam, scene = stream_files
    exe = str(d / "stereo_prior")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_stereo_prior.cpp"), "-o", exe, "-L", host_lib, "-lrebvio", "-lrebvio_hip",
                    f"-Wl,-rpath,{host_lib}", "-pthread"], check=True)
    r = subprocess.run([exe, str(lp), str(rp), str(W), str(H), str(N), repr(cam.fm), repr(cam.cx), repr(cam.cy), "600", "800", str(ip), "50",
                        repr(BASELINE), repr(scene.z_front), repr(scene.z_back)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-6000:], r.stderr[-2000:])


@pytest.mark.gpu
def test_replay_reads_a_raw_right_file(host_lib, stream_files):
    """--right FILE --baseline B: every frame's right image is fused (none dropped); the two options come together"""
    d, lp, rp, ip, cam, _ = stream_files
    odo0, odo1 = d / "odometry0.txt", d / "odometry1.txt"
    base = [os.path.join(host_lib, "rebvio_replay"), "--raw", str(lp), "--size", str(W), str(H), "--imu", str(ip), "--camera", repr(cam.fm),
            repr(cam.cx), repr(cam.cy), "--keylines", "600", "800", "--min-matches", "50"]
    r0 = subprocess.run(base + ["--out", str(odo0)], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and "right_images" not in r0.stderr, (r0.stdout, r0.stderr[-2000:])
    r = subprocess.run(base + ["--out", str(odo1), "--right", str(rp), "--baseline", repr(BASELINE)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert f"right_images={N} stereo_fused_frames={N} " in r.stderr and "right_dropped=0" in r.stderr, r.stderr[-2000:]
    assert len(open(odo1).read().splitlines()) == len(open(odo0).read().splitlines())
    for bad in (["--right", str(rp)], ["--baseline", "0.2"], ["--right", str(rp), "--baseline", "0"], ["--right", str(d / "missing.u8"), "--baseline", "0.2"]):
        b = subprocess.run(base + ["--out", str(odo1)] + bad, capture_output=True, text=True, timeout=60)
        assert b.returncode in (1, 2), (bad, b.returncode, b.stderr[-500:])
