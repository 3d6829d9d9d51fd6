"""rebvio::Rebvio::setKeyframeWindow / registerKeyframeWindowCallback, EdgeMap::keyframeAlignMany and the free functions
keyframeAlignBest / keyframeHypothesesAround (tests/cpp/test_keyframe_window.cpp says what it checks), and the file
`rebvio_replay --kf-window` writes, on the GPU."""
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
    d = tmp_path_factory.mktemp("kfwindow")
    frames, cam = synth.render_stream(W, H, N)
    ts, gyro, acc = synth.imu_samples(synth.make_scene(0), N, noise_seed=1)
    fp, ip = d / "frames.u8", d / "imu.bin"
    frames.tofile(fp)
    rec = np.zeros(len(ts), dtype=[("ts", "<i8"), ("gyro", "<f4", 3), ("acc", "<f4", 3)])
    rec["ts"], rec["gyro"], rec["acc"] = ts, gyro, acc
    rec.tofile(ip)
    return d, fp, ip, cam


def test_keyframe_window_and_edge_map_entries(host_lib, stream_files):
    d, fp, ip, cam = stream_files
    exe = str(d / "keyframe_window")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_keyframe_window.cpp"), "-o", exe, "-L", host_lib, "-lrebvio", "-lrebvio_hip",
                    f"-Wl,-rpath,{host_lib}", "-pthread"], check=True)
    r = subprocess.run([exe, str(fp), str(W), str(H), str(N), repr(cam.fm), repr(cam.cx), repr(cam.cy), "600", "800", str(ip), "50", "3"],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-8000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-8000:], r.stderr[-2000:])


def test_replay_writes_the_window_file(host_lib, stream_files):
    """the format of --kf-window: ts_us kf_ts_us status used inliers R[9] t[3], one line per (record, keyframe), the current keyframe
    first; the odometry file and the --kf-align file do not change by a byte; the flag needs --kf-align"""
    d, fp, ip, cam = stream_files
    odo, poses, win = d / "odometry.txt", d / "kf_align.txt", d / "kf_window.txt"
    odo0, poses0 = d / "odometry_plain.txt", d / "kf_align_plain.txt"
    base = [os.path.join(host_lib, "rebvio_replay"), "--raw", str(fp), "--size", str(W), str(H), "--imu", str(ip), "--camera", repr(cam.fm),
            repr(cam.cx), repr(cam.cy), "--keylines", "600", "800", "--min-matches", "50", "--kf-every", "3"]
    r = subprocess.run(base + ["--out", str(odo0), "--kf-align", str(poses0)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    r = subprocess.run(base + ["--out", str(odo), "--kf-align", str(poses), "--kf-window", "3", str(win)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    lines = open(win).read().splitlines()
    assert f"kf_window_lines={len(lines)}" in r.stderr, r.stderr[-2000:]
    pose_lines = open(poses).read().splitlines()
    assert len(pose_lines) == N - 1 == len(open(odo).read().splitlines())
    by_ts, order = {}, []
    for line in lines:
        f = line.split()
        assert len(f) == 17, line
        ts, kf_ts, status, used, inl = (int(x) for x in f[:5])
        v = np.array([float(x) for x in f[5:]])
        assert kf_ts <= ts and status in (0, 2, 3) and 0 <= inl <= used and np.isfinite(v).all(), line
        assert [repr(float(x)) for x in f[5:]] == [repr(x) for x in v.tolist()]     # (%.17g: every double reads back exactly)
        if ts not in by_ts:
            order.append(ts)
        by_ts.setdefault(ts, []).append((kf_ts, status, used, f[5:]))
    assert order == [(k + 1) * 50000 for k in range(N - 1)]                          # every record has its entries, in record order
    for k, ts in enumerate(order):
        entries = by_ts[ts]
        assert 1 <= len(entries) <= 4, (ts, len(entries))
        assert [e[0] for e in entries] == sorted({e[0] for e in entries}, reverse=True)      # the current keyframe, then newest first
        p = pose_lines[k].split()                                                   # the first entry is the --kf-align file's line
        assert [int(p[0]), int(p[1]), int(p[2])] == [ts, entries[0][1], entries[0][2]] and p[3:] == entries[0][3], (ts, pose_lines[k])
    assert max(len(by_ts[ts]) for ts in order) >= 2
    print("\n".join(" ".join(line.split()[:5]) for line in lines))
    # (the requests come from the odometry callback on the state-estimation thread itself: they land on the same records in every run)
    assert open(odo0).read() == open(odo).read() and open(poses0).read() == open(poses).read()
    # the flag needs --kf-align FILE, a window of 1..15, and comes once
    for bad in (["--kf-window", "3", str(win)], ["--kf-pose", str(poses), "--kf-window", "3", str(win)],
                ["--kf-align", str(poses), "--kf-window", "0", str(win)], ["--kf-align", str(poses), "--kf-window", "16", str(win)],
                ["--kf-align", str(poses), "--kf-window", "3", str(win), "--kf-window", "3", str(win)]):
        b = subprocess.run(base + ["--out", str(odo)] + bad, capture_output=True, text=True, timeout=60)
        assert b.returncode == 2 and "usage" in b.stderr, (bad, b.returncode, b.stderr[-500:])
