"""rebvio::Rebvio::setKeyframeAlign, KeyframeSnapshot::addNormals / EdgeMap::keyframeAlign (tests/cpp/test_keyframe_align.cpp says what
it checks) and the file `rebvio_replay --kf-align` writes, on the GPU."""
import os
import subprocess

import numpy as np
import pytest

from support import host_lib  # noqa: F401
from support import ROOT


pytestmark = pytest.mark.gpu

N, W, H = 20, 160, 120


@pytest.fixture(scope="module")
def stream_files(tmp_path_factory):
    from rebvio_amd import synth
    d = tmp_path_factory.mktemp("kfalign")
    frames, cam = synth.render_stream(W, H, N)
    ts, gyro, acc = synth.imu_samples(synth.make_scene(0), N, noise_seed=1)
    fp, ip = d / "frames.u8", d / "imu.bin"
    frames.tofile(fp)
    rec = np.zeros(len(ts), dtype=[("ts", "<i8"), ("gyro", "<f4", 3), ("acc", "<f4", 3)])
    rec["ts"], rec["gyro"], rec["acc"] = ts, gyro, acc
    rec.tofile(ip)
    return d, fp, ip, cam


def test_set_keyframe_align_and_edge_map_entries(host_lib, stream_files):
    d, fp, ip, cam = stream_files
    exe = str(d / "keyframe_align")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_keyframe_align.cpp"), "-o", exe, "-L", host_lib, "-lrebvio", "-lrebvio_hip",
                    f"-Wl,-rpath,{host_lib}", "-pthread"], check=True)
    r = subprocess.run([exe, str(fp), str(W), str(H), str(N), repr(cam.fm), repr(cam.cx), repr(cam.cy), "600", "800", str(ip), "50", "5"],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-6000:], r.stderr[-2000:])


def test_replay_writes_the_pose_file_from_the_alignment(host_lib, stream_files):
    """the format of --kf-pose: ts_us status used R[9] t[3], one line per record; the odometry file does not change by a byte"""
    d, fp, ip, cam = stream_files
    odo, poses, plain = d / "odometry.txt", d / "kf_align.txt", d / "odometry_plain.txt"
    base = [os.path.join(host_lib, "rebvio_replay"), "--raw", str(fp), "--size", str(W), str(H), "--imu", str(ip), "--camera", repr(cam.fm),
            repr(cam.cx), repr(cam.cy), "--keylines", "600", "800", "--min-matches", "50"]
    r = subprocess.run(base + ["--out", str(odo), "--kf-align", str(poses), "--kf-every", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert f"kf_poses={N - 1}" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["--out", str(plain)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert open(odo).read() == open(plain).read()
    lines = open(poses).read().splitlines()
    assert len(lines) == N - 1 == len(open(odo).read().splitlines())
    good = 0
    for k, line in enumerate(lines):
        f = line.split()
        assert len(f) == 15, line
        ts, status, used = int(f[0]), int(f[1]), int(f[2])
        v = np.array([float(x) for x in f[3:]])
        assert ts == (k + 1) * 50000 and status in (0, 2, 3) and used >= 0 and np.isfinite(v).all(), line
        assert [repr(float(x)) for x in f[3:]] == [repr(x) for x in v.tolist()]     # (%.17g: every double reads back exactly)
        if status == 0:
            assert np.abs(v[:9].reshape(3, 3) @ v[:9].reshape(3, 3).T - np.eye(3)).max() < 1e-12 and used >= 12, line
            good += 1
    print("\n".join(" ".join(line.split()[:3]) for line in lines))
    assert good > 0
    for extra in (["--kf-pose", str(poses)], ["--kf-align", str(poses)]):      # one of the two, once
        bad = subprocess.run(base + ["--out", str(odo), "--kf-align", str(poses)] + extra, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and "usage" in bad.stderr
