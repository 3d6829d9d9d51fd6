"""rebvio::Rebvio::registerKeyframeCloudCallback, KeyframeSnapshot::pointCloud (tests/cpp/test_keyframe_cloud.cpp says what it
checks) and the files `rebvio_replay --kf-cloud` writes, on the GPU."""
import glob
import os
import re
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
    d = tmp_path_factory.mktemp("kfcloud")
    frames, cam = synth.render_stream(W, H, N)
    ts, gyro, acc = synth.imu_samples(synth.make_scene(0), N, noise_seed=1)
    fp, ip = d / "frames.u8", d / "imu.bin"
    frames.tofile(fp)
    rec = np.zeros(len(ts), dtype=[("ts", "<i8"), ("gyro", "<f4", 3), ("acc", "<f4", 3)])
    rec["ts"], rec["gyro"], rec["acc"] = ts, gyro, acc
    rec.tofile(ip)
    return d, fp, ip, cam


@pytest.fixture(scope="module")
def exe(host_lib, stream_files):
    path = str(stream_files[0] / "keyframe_cloud")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_keyframe_cloud.cpp"), "-o", path, "-L", host_lib, "-lrebvio", "-lrebvio_hip",
                    f"-Wl,-rpath,{host_lib}", "-pthread"], check=True)
    return path


def test_keyframe_cloud_callback_and_snapshot_point_cloud(exe, stream_files):
    d, fp, ip, cam = stream_files
    r = subprocess.run([exe, str(fp), str(W), str(H), str(N), repr(cam.fm), repr(cam.cx), repr(cam.cy), "600", "800", str(ip), "50", "5", "10", "15"],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-6000:], r.stderr[-2000:])


def test_replay_writes_one_ply_per_retired_keyframe(exe, host_lib, stream_files):
    """--kf-cloud PREFIX: one PLY per retired keyframe, named by the keyframe's stamp; io::readPointCloudPly reads them back to the
    point counts the callback saw; with --kf-fuse too; the odometry file does not change"""
    d, fp, ip, cam = stream_files
    base = [os.path.join(host_lib, "rebvio_replay"), "--raw", str(fp), "--size", str(W), str(H), "--imu", str(ip), "--camera", repr(cam.fm),
            repr(cam.cx), repr(cam.cy), "--keylines", "600", "800", "--min-matches", "50"]
    plain = d / "odometry_plain.txt"
    r0 = subprocess.run(base + ["--out", str(plain)], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and "kf_clouds" not in r0.stderr, (r0.stdout, r0.stderr[-2000:])
    for name, extra in (("marked", []), ("fused", ["--kf-fuse", str(d / "kf_fuse.txt"), "--kf-align", str(d / "kf_align.txt")])):
        odo, prefix = d / f"odometry_{name}.txt", str(d / f"{name}_kf_")
        r = subprocess.run(base + ["--out", str(odo), "--kf-cloud", prefix, "--kf-every", "4"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
        assert open(odo).read() == open(plain).read()
        m = re.search(r"kf_clouds=(\d+) kf_points=(\d+)", r.stderr)
        assert m, r.stderr[-2000:]
        n_clouds, n_points = int(m.group(1)), int(m.group(2))
        files = sorted(glob.glob(prefix + "*.ply"), key=lambda p: int(p[len(prefix):-4]))
        # a keyframe before the first frame and one requested from the callback of every 4th of the 19 records: every one of them but
        # the last is retired, whichever pair a request lands on
        assert len(files) == n_clouds and 3 <= n_clouds <= 4, (files, r.stderr[-2000:])
        back = subprocess.run([exe, "--read-ply"] + files, capture_output=True, text=True, timeout=60)
        assert back.returncode == 0, back.stdout
        rows = [[int(x) for x in line.split()] for line in back.stdout.splitlines()]
        print(name, rows)
        assert [ts for ts, _ in rows] == [int(p[len(prefix):-4]) for p in files]          # the stamp in the name is the one in the file
        assert all(ts % 50000 == 0 and ts < (N - 1) * 50000 for ts, _ in rows)
        assert sum(n for _, n in rows) == n_points and n_points > 0
