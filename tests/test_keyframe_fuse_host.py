"""rebvio::Rebvio::setKeyframeDepthFusion / registerKeyframeFuseCallback, KeyframeSnapshot::fuseDepth (tests/cpp/test_keyframe_fuse.cpp
says what it checks) and the file `rebvio_replay --kf-fuse` writes, on the GPU."""
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
    d = tmp_path_factory.mktemp("kffuse")
    frames, cam = synth.render_stream(W, H, N)
    ts, gyro, acc = synth.imu_samples(synth.make_scene(0), N, noise_seed=1)
    fp, ip = d / "frames.u8", d / "imu.bin"
    frames.tofile(fp)
    rec = np.zeros(len(ts), dtype=[("ts", "<i8"), ("gyro", "<f4", 3), ("acc", "<f4", 3)])
    rec["ts"], rec["gyro"], rec["acc"] = ts, gyro, acc
    rec.tofile(ip)
    return d, fp, ip, cam


def test_set_keyframe_depth_fusion_and_fuse_depth(host_lib, stream_files):
    d, fp, ip, cam = stream_files
    exe = str(d / "keyframe_fuse")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_keyframe_fuse.cpp"), "-o", exe, "-L", host_lib, "-lrebvio", "-lrebvio_hip",
                    f"-Wl,-rpath,{host_lib}", "-pthread"], check=True)
    r = subprocess.run([exe, str(fp), str(W), str(H), str(N), repr(cam.fm), repr(cam.cx), repr(cam.cy), "600", "800", str(ip), "50", "5", "12"],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-6000:], r.stderr[-2000:])


def test_replay_writes_the_fuse_file(host_lib, stream_files):
    """--kf-fuse: ts_us candidates associated fused gated flat clamped, one line per pose record of status 0 other than a keyframe's
    own; it implies the alignment, whose pose file does not depend on how it was asked for; the odometry file does not change"""
    d, fp, ip, cam = stream_files
    odo, fuse, poses, plain, fuse2 = d / "odometry.txt", d / "kf_fuse.txt", d / "kf_align.txt", d / "odometry_plain.txt", d / "kf_fuse2.txt"
    base = [os.path.join(host_lib, "rebvio_replay"), "--raw", str(fp), "--size", str(W), str(H), "--imu", str(ip), "--camera", repr(cam.fm),
            repr(cam.cx), repr(cam.cy), "--keylines", "600", "800", "--min-matches", "50"]
    r = subprocess.run(base + ["--out", str(odo), "--kf-fuse", str(fuse), "--kf-align", str(poses), "--kf-every", "4"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert f"kf_poses={N - 1}" in r.stderr, r.stderr[-2000:]
    r2 = subprocess.run(base + ["--out", str(plain), "--kf-fuse", str(fuse2), "--kf-every", "4"], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and f"kf_poses={N - 1}" in r2.stderr, (r2.stdout, r2.stderr[-2000:])
    alone = open(fuse2).read().splitlines()                        # --kf-fuse alone aligns too
    assert len(alone) > 0 and all(len(line.split()) == 7 for line in alone) and f"kf_fusions={len(alone)}" in r2.stderr
    r3 = subprocess.run(base + ["--out", str(plain)], capture_output=True, text=True, timeout=300)
    assert r3.returncode == 0, (r3.stdout, r3.stderr[-2000:])
    assert open(odo).read() == open(plain).read()
    pose_lines = [line.split() for line in open(poses).read().splitlines()]
    assert len(pose_lines) == N - 1
    # a keyframe is requested before the first frame (its own record is the first one) and from the callback of every 4th record;
    # which pair such a request lands on is the pipeline's business (tests/cpp/test_keyframe_fuse.cpp pins it with waitIdle)
    ok_ts = [int(p[0]) for p in pose_lines if int(p[1]) == 0]
    lines = open(fuse).read().splitlines()
    print("\n".join(lines))
    assert f"kf_fusions={len(lines)}" in r.stderr, r.stderr[-2000:]
    got_ts = [int(line.split()[0]) for line in lines]
    assert got_ts == sorted(set(got_ts)) and set(got_ts) <= set(ok_ts) and int(pose_lines[0][0]) not in got_ts and len(got_ts) > 0
    assert 1 <= len(ok_ts) - len(got_ts) <= 1 + (N - 1) // 4          # the keyframes' own records, and nothing else, are left out
    for line in lines:
        f = [int(x) for x in line.split()]
        assert len(f) == 7, line
        ts, cand, assoc, fused, gated, flat, clamped = f
        assert 0 < cand <= 800 and assoc == fused + gated + flat and assoc <= cand and 0 <= clamped <= fused and min(fused, gated, flat) >= 0, line
    assert sum(int(line.split()[3]) for line in lines) > 0
    bad = subprocess.run(base + ["--out", str(odo), "--kf-pose", str(poses), "--kf-fuse", str(fuse)], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "usage" in bad.stderr          # the chain pose has no fusion behind it
    bad = subprocess.run(base + ["--out", str(odo), "--kf-fuse", str(fuse), "--kf-fuse", str(fuse)], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "usage" in bad.stderr
