"""rebvio::EdgeMap::edgeSegments, rebvio::Rebvio::registerEdgeSegmentCallback, io::writeSegmentsPly / readSegmentsPly
(tests/cpp/test_edge_segments.cpp says what it checks) and the files `rebvio_replay --segments` writes, on the GPU."""
import glob
import os
import subprocess

import numpy as np
import pytest

from support import host_lib  # noqa: F401
from support import ROOT


pytestmark = pytest.mark.gpu

N, W, H = 12, 160, 120


@pytest.fixture(scope="module")
def stream_files(tmp_path_factory):
    from rebvio_amd import synth
    d = tmp_path_factory.mktemp("edgesegments")
    frames, cam = synth.render_stream(W, H, N)
    ts, gyro, acc = synth.imu_samples(synth.make_scene(0), N, noise_seed=1)
    fp, ip = d / "frames.u8", d / "imu.bin"
    frames.tofile(fp)
    rec = np.zeros(len(ts), dtype=[("ts", "<i8"), ("gyro", "<f4", 3), ("acc", "<f4", 3)])
    rec["ts"], rec["gyro"], rec["acc"] = ts, gyro, acc
    rec.tofile(ip)
    return d, fp, ip, cam


def test_classes_callback_and_ply_round_trip(host_lib, stream_files):
    d, fp, ip, cam = stream_files
    exe = str(d / "edge_segments")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_edge_segments.cpp"), "-o", exe, "-L", host_lib, "-lrebvio", "-lrebvio_hip",
                    f"-Wl,-rpath,{host_lib}", "-pthread"], check=True)
    r = subprocess.run([exe, str(fp), str(W), str(H), str(N), repr(cam.fm), repr(cam.cx), repr(cam.cy), "600", "800", str(ip), "50", str(d)],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-6000:], r.stderr[-2000:])


def read_segments_ply(path):
    """(ts_us, vertices float32 [n, 4], edges int32 [m, 2]) of a file of io::writeSegmentsPly"""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"] and lines[2].startswith("comment rebvio segments ts_us "), lines
    assert lines[4:8] == ["property float x", "property float y", "property float z", "property float intensity"]
    assert lines[9:] == ["property int vertex1", "property int vertex2"], lines
    n, m = int(lines[3].split()[-1]), int(lines[8].split()[-1])
    assert lines[3] == f"element vertex {n}" and lines[8] == f"element edge {m}" and len(body) == 16 * n + 8 * m
    return int(lines[2].split()[-1]), np.frombuffer(body[:16 * n], "<f4").reshape(n, 4), np.frombuffer(body[16 * n:], "<i4").reshape(m, 2)


def test_replay_writes_the_segment_files(host_lib, stream_files):
    """--segments PREFIX [--seg-tol T]: one PLY file per record, two vertices and one edge per depth-valid segment; the odometry file is
    what it is without the flag; a tighter tolerance splits more; a missing, repeated or out-of-range argument is exit status 2"""
    d, fp, ip, cam = stream_files
    odo, odo0 = d / "odometry.txt", d / "odometry0.txt"
    base = [os.path.join(host_lib, "rebvio_replay"), "--raw", str(fp), "--size", str(W), str(H), "--imu", str(ip), "--camera", repr(cam.fm),
            repr(cam.cx), repr(cam.cy), "--keylines", "600", "800", "--min-matches", "50"]
    r0 = subprocess.run(base + ["--out", str(odo0)], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and "segment_files" not in r0.stderr, (r0.stdout, r0.stderr[-2000:])
    totals = {}
    for tol in (None, "0.3"):
        prefix = str(d / f"segs{tol}_")
        r = subprocess.run(base + ["--out", str(odo), "--segments", prefix, "--min-chain", "4"] + (["--seg-tol", tol] if tol else []),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
        assert open(odo).read() == open(odo0).read()
        files = sorted(glob.glob(prefix + "*.ply"), key=lambda p: int(p[len(prefix):-4]))
        assert [int(p[len(prefix):-4]) for p in files] == [50000 * k for k in range(1, N)]
        n_edges = 0
        for p in files:
            ts, v, e = read_segments_ply(p)
            assert ts == int(p[len(prefix):-4]) and np.isfinite(v).all() and len(v) == 2 * len(e)
            assert np.array_equal(e, np.arange(2 * len(e), dtype=np.int32).reshape(-1, 2))
            assert (v[:, 3] >= 0).all()      # intensity: the end's sigma_rho
            n_edges += len(e)
        assert f"segment_files={N - 1} " in r.stderr and f"segments_valid={n_edges}" in r.stderr, r.stderr[-2000:]
        totals[tol] = n_edges
    print(totals)
    assert totals[None] > 0 and totals["0.3"] > 0
    for bad in (["--segments"], ["--segments", "a", "--segments", "b"], ["--segments", "a", "--seg-tol"], ["--segments", "a", "--seg-tol", "-1"],
                ["--segments", "a", "--seg-tol", "nan"], ["--segments", "a", "--seg-tol", "abc"], ["--segments", "a", "--seg-tol", "1x"], ["--segments", "a", "--seg-tol", "1", "--seg-tol", "2"], ["--seg-tol", "1"],
                ["--segments", "a", "--seg-tol", "1e9"]):
        b = subprocess.run(base + ["--out", str(odo)] + bad, capture_output=True, text=True, timeout=60)
        assert b.returncode == 2, (bad, b.returncode, b.stderr[-500:])
