"""rebvio::Rebvio's keyframe-pose callback, EdgeMap::keyframeSnapshot / keyframePose (tests/cpp/test_keyframe_pose.cpp says what it
checks) and the file `rebvio_replay --kf-pose` writes, on the GPU."""
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
    d = tmp_path_factory.mktemp("kfpose")
    frames, cam = synth.render_stream(W, H, N)
    ts, gyro, acc = synth.imu_samples(synth.make_scene(0), N, noise_seed=1)
    fp, ip = d / "frames.u8", d / "imu.bin"
    frames.tofile(fp)
    rec = np.zeros(len(ts), dtype=[("ts", "<i8"), ("gyro", "<f4", 3), ("acc", "<f4", 3)])
    rec["ts"], rec["gyro"], rec["acc"] = ts, gyro, acc
    rec.tofile(ip)
    return d, fp, ip, cam


def test_pose_callback_and_edge_map_entries(host_lib, stream_files):
    d, fp, ip, cam = stream_files
    exe = str(d / "keyframe_pose")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_keyframe_pose.cpp"), "-o", exe, "-L", host_lib, "-lrebvio", "-lrebvio_hip",
                    f"-Wl,-rpath,{host_lib}", "-pthread"], check=True)
    r = subprocess.run([exe, str(fp), str(W), str(H), str(N), repr(cam.fm), repr(cam.cx), repr(cam.cy), "600", "800", str(ip), "50", "5"],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-4000:], r.stderr[-2000:])


def test_replay_writes_one_pose_line_per_record(host_lib, stream_files):
    """ts_us status used R[9] t[3]; a keyframe is requested before the first frame and after every fourth record, so every record has
    a pose line and the estimate returns to the identity several times"""
    d, fp, ip, cam = stream_files
    odo, poses, plain = d / "odometry.txt", d / "kf_pose.txt", d / "odometry_plain.txt"
    base = [os.path.join(host_lib, "rebvio_replay"), "--raw", str(fp), "--size", str(W), str(H), "--imu", str(ip), "--camera", repr(cam.fm),
            repr(cam.cx), repr(cam.cy), "--keylines", "600", "800", "--min-matches", "50"]
    r = subprocess.run(base + ["--out", str(odo), "--kf-pose", str(poses), "--kf-every", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert f"kf_poses={N - 1}" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["--out", str(plain)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert open(odo).read() == open(plain).read()           # the odometry file does not change by a byte
    lines = open(poses).read().splitlines()
    assert len(lines) == N - 1 == len(open(odo).read().splitlines())
    identities = 0
    for k, line in enumerate(lines):
        f = line.split()
        assert len(f) == 15, line
        ts, status, used = int(f[0]), int(f[1]), int(f[2])
        v = np.array([float(x) for x in f[3:]])
        assert ts == (k + 1) * 50000 and status in (0, 2, 3) and used >= 0 and np.isfinite(v).all(), line
        assert [repr(float(x)) for x in f[3:]] == [repr(x) for x in v.tolist()]     # (%.17g: every double reads back exactly)
        R, t = v[:9].reshape(3, 3), v[9:]
        if status == 0:
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12, line
        identities += bool(status == 0 and np.abs(R - np.eye(3)).max() <= 1e-9 and np.abs(t).max() <= 1e-9)
    # The first record's map is the first keyframe: its pose is the identity. It has been a new map once, so none of its keylines has the
    # two matches the default filter asks for: status 3 (pose = guess) until the next keyframe. Further keyframes follow the 4th, 8th,
    # 12th and 16th record (the request is seen by the pair being tracked at that moment, so their exact records depend on the
    # threads' timing): each starts at the identity with status 0.
    assert [float(x) for x in lines[0].split()[3:]] == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    assert 2 <= identities <= 5, identities
    assert {int(line.split()[1]) for line in lines[7:]} == {0}
    bad = subprocess.run(base + ["--out", str(odo), "--kf-pose", str(poses), "--kf-every", "0"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "usage" in bad.stderr
