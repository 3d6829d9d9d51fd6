"""rebvio::Rebvio::setKeyframeDepthHandover / registerKeyframeHandoverCallback, KeyframeSnapshot::handoverDepth
(tests/cpp/test_keyframe_handover.cpp says what it checks) and the file `rebvio_replay --kf-handover` writes, on the GPU."""
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
    d = tmp_path_factory.mktemp("kfhandover")
    frames, cam = synth.render_stream(W, H, N)
    ts, gyro, acc = synth.imu_samples(synth.make_scene(0), N, noise_seed=1)
    fp, ip = d / "frames.u8", d / "imu.bin"
    frames.tofile(fp)
    rec = np.zeros(len(ts), dtype=[("ts", "<i8"), ("gyro", "<f4", 3), ("acc", "<f4", 3)])
    rec["ts"], rec["gyro"], rec["acc"] = ts, gyro, acc
    rec.tofile(ip)
    return d, fp, ip, cam


def test_set_keyframe_depth_handover_and_handover_depth(host_lib, stream_files):
    d, fp, ip, cam = stream_files
    exe = str(d / "keyframe_handover")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_keyframe_handover.cpp"), "-o", exe, "-L", host_lib, "-lrebvio", "-lrebvio_hip",
                    f"-Wl,-rpath,{host_lib}", "-pthread"], check=True)
    r = subprocess.run([exe, str(fp), str(W), str(H), str(N), repr(cam.fm), repr(cam.cx), repr(cam.cy), "600", "800", str(ip), "50", "5", "12"],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-6000:], r.stderr[-2000:])


def test_replay_writes_the_handover_file(host_lib, stream_files):
    """--kf-handover: ts_us kf_ts_us and the seven counts, one line per hand-over; it needs --kf-align; the odometry file does not change,
    and the pose and fuse files are what they are without the flag up to the first hand-over"""
    d, fp, ip, cam = stream_files
    odo, ho, poses, fuse = d / "odometry.txt", d / "kf_handover.txt", d / "kf_align.txt", d / "kf_fuse.txt"
    odo0, poses0, fuse0 = d / "odometry0.txt", d / "kf_align0.txt", d / "kf_fuse0.txt"
    base = [os.path.join(host_lib, "rebvio_replay"), "--raw", str(fp), "--size", str(W), str(H), "--imu", str(ip), "--camera", repr(cam.fm),
            repr(cam.cx), repr(cam.cy), "--keylines", "600", "800", "--min-matches", "50"]
    r = subprocess.run(base + ["--out", str(odo), "--kf-align", str(poses), "--kf-fuse", str(fuse), "--kf-handover", str(ho), "--kf-every", "4"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    r0 = subprocess.run(base + ["--out", str(odo0), "--kf-align", str(poses0), "--kf-fuse", str(fuse0), "--kf-every", "4"], capture_output=True,
                        text=True, timeout=300)
    assert r0.returncode == 0 and "kf_handovers" not in r0.stderr, (r0.stdout, r0.stderr[-2000:])
    assert open(odo).read() == open(odo0).read()
    lines = open(ho).read().splitlines()
    print("\n".join(lines))
    assert f"kf_handovers={len(lines)}" in r.stderr and len(lines) > 0, r.stderr[-2000:]
    pose_lines = [line.split() for line in open(poses).read().splitlines()]
    pose_ts = [int(p[0]) for p in pose_lines]
    assert len(pose_lines) == N - 1
    # a keyframe is requested before the first frame and from the callback of every 4th record; which pair such a request lands on is
    # the pipeline's business (tests/cpp/test_keyframe_handover.cpp pins it with waitIdle): at most one hand-over per request
    assert len(lines) <= (N - 1) // 4
    seen = []
    for line in lines:
        f = [int(x) for x in line.split()]
        assert len(f) == 9, line
        ts, kf_ts, cand, assoc, oor, claimed, adopted, kept, conflicts = f
        assert ts in pose_ts and kf_ts in pose_ts and kf_ts < ts, line
        assert 0 < cand <= 800 and assoc <= cand and claimed == adopted + kept + conflicts and assoc - oor - claimed >= 0, line
        assert min(oor, adopted, kept, conflicts) >= 0, line
        seen.append((ts, kf_ts))
    assert [s[0] for s in seen] == sorted({s[0] for s in seen})        # one per record at most, in order
    # the other output files are what they are without the flag up to (and including) the record of the first hand-over
    first = seen[0][0]
    cut = lambda path: [line for line in open(path).read().splitlines() if int(line.split()[0]) <= first]
    assert cut(poses) == cut(poses0) and cut(fuse) == cut(fuse0) and len(cut(poses)) > 0
    for bad in (["--kf-handover", str(ho)], ["--kf-pose", str(poses), "--kf-handover", str(ho)], ["--kf-fuse", str(fuse), "--kf-handover", str(ho)],
                ["--kf-align", str(poses), "--kf-handover", str(ho), "--kf-handover", str(ho)]):
        b = subprocess.run(base + ["--out", str(odo)] + bad, capture_output=True, text=True, timeout=60)
        assert b.returncode == 2 and "usage" in b.stderr, (bad, b.returncode, b.stderr[-500:])
