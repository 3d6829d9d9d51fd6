"""rebvio::Rebvio's point-cloud callback, EdgeMap::pointCloud and rebvio_replay --cloud on the GPU
(tests/cpp/test_point_cloud.cpp says what it checks)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from support import host_lib  # noqa: F401
from support import ROOT


pytestmark = pytest.mark.gpu


def _write_imu(path, ts, gyro, acc):
    rec = np.zeros(len(ts), dtype=[("ts", "<i8"), ("gyro", "<f4", 3), ("acc", "<f4", 3)])
    rec["ts"], rec["gyro"], rec["acc"] = ts, gyro, acc
    rec.tofile(path)


def test_point_cloud_callback_and_replay_ply_files(host_lib, tmp_path):
    from rebvio_amd import synth
    n, W, H = 40, 320, 240
    frames, cam = synth.render_stream(W, H, n)
    ts, gyro, acc = synth.imu_samples(synth.make_scene(0), n, noise_seed=1)
    fp, ip = tmp_path / "frames.u8", tmp_path / "imu.bin"
    frames.tofile(fp)
    _write_imu(ip, ts, gyro, acc)
    exe = str(tmp_path / "point_cloud")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_point_cloud.cpp"), "-o", exe, "-L", host_lib, "-lrebvio", "-lrebvio_hip",
                    f"-Wl,-rpath,{host_lib}", "-pthread"], check=True)
    summary = tmp_path / "summary.txt"
    r = subprocess.run([exe, str(fp), str(W), str(H), str(n), repr(cam.fm), repr(cam.cx), repr(cam.cy), "3000", "4000", str(ip), "100",
                        str(summary)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-3000:], r.stderr[-2000:])
    want = [ln.split() for ln in open(summary).read().splitlines()]
    assert len(want) == n - 1

    # rebvio_replay --cloud: one PLY per published record; vertex count, first and last vertex equal the callback's
    prefix = str(tmp_path / "cloud_")
    r = subprocess.run([os.path.join(host_lib, "rebvio_replay"), "--raw", str(fp), "--size", str(W), str(H), "--imu", str(ip), "--camera",
                        repr(cam.fm), repr(cam.cx), repr(cam.cy), "--keylines", "3000", "4000", "--min-matches", "100",
                        "--out", str(tmp_path / "odometry.txt"), "--cloud", prefix], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"clouds={n - 1}" in r.stderr, (r.returncode, r.stderr[-2000:])
    files = sorted(f for f in os.listdir(tmp_path) if f.startswith("cloud_") and f.endswith(".ply"))
    assert len(files) == n - 1
    nonempty = 0
    for rec in want:
        raw = open(f"{prefix}{rec[0]}.ply", "rb").read()
        head, body = raw.split(b"end_header\n", 1)
        lines = head.decode().splitlines()
        assert lines[:2] == ["ply", "format binary_little_endian 1.0"] and lines[2].endswith(f"ts_us {rec[0]}")
        assert lines[3] == f"element vertex {rec[1]}"
        assert lines[4:] == ["property float x", "property float y", "property float z", "property float intensity"]
        count = int(rec[1])
        assert len(body) == 16 * count
        if count:
            nonempty += 1
            words = struct.unpack(f"<{4 * count}I", body)
            assert [f"{w:08x}" for w in words[:4]] == rec[2:6], rec[0]
            assert [f"{w:08x}" for w in words[-4:]] == rec[6:10], rec[0]
            assert np.isfinite(np.frombuffer(body, "<f4")).all()
    assert nonempty >= n - 1 - 6
