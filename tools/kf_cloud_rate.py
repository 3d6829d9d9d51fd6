#!/usr/bin/env python3
"""What the point cloud of a keyframe snapshot costs.  One JSON line per measurement on stdout.

  kernels   device time per launch of k_kf_cloud_count / k_kf_cloud_emit next to k_cloud_count / k_cloud_emit in the same process
            (rebvio_hip_profile_*: HIP events around every launch), alternating, three rounds of `--reps` calls each, and the wall
            time of the synchronous rebvio_hip_kf_snapshot_point_cloud call next to rebvio_hip_map_point_cloud, on the two scenes of
            tools/kf_align_rate.py: the 16 000-keyline snapshot of the 640x480 bench stream against that stream's map seven pairs on,
            and a 65 536-keyline snapshot against the 65 536-keyline map it was taken from
  host      rebvio::Rebvio (rebvio_replay) on the bench stream with --kf-every 10 --kf-fuse, without and with --kf-cloud, processes
            alternating, `--rounds` times each; the option's price as the ratio of the median rates

    tools/kf_cloud_rate.py [kernels] [host] [--frames N] [--rounds R] [--reps K]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAMES = ("k_kf_cloud_count", "k_kf_cloud_emit", "k_cloud_count", "k_cloud_emit", "k_cloud_copy")


def wall(call, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    return round((time.perf_counter() - t0) / reps * 1e6, 1)


def time_pair(B, ctx, snap, m, reps, what):
    n_map, n_snap = m.size(), len(snap.download()[0])
    flt = B.default_cloud_filter()
    _, c_map = m.point_cloud(flt, return_count=True)           # warm: buffers allocated
    _, c_snap = snap.point_cloud(flt, return_count=True)
    out = dict(what=what, map_keylines=n_map, map_points=c_map, snapshot_keylines=n_snap, snapshot_points=c_snap, reps=reps)
    calls = (("snapshot", lambda: snap.point_cloud(flt, cap=n_snap)), ("map", lambda: m.point_cloud(flt, cap=n_map)))
    for _ in range(3):                                         # the two extractions alternating, three rounds: the table's own spread
        for kind, call in calls:
            ctx.profile(True, only="k_*")
            ctx.profile_reset()
            for _ in range(reps):
                call()
            prof = ctx.profile_read()
            ctx.profile(False)
            for name in NAMES:
                if name in prof and prof[name][1]:
                    key = name + "_us" if name != "k_cloud_copy" else f"k_cloud_copy_behind_{kind}_us"
                    out.setdefault(key, []).append(round(prof[name][0], 2))
    for _ in range(3):
        for kind, call in calls:
            out.setdefault(kind + "_sync_call_wall_us", []).append(wall(call, reps))
    print(json.dumps(out), flush=True)


def kernels(args):
    import torch  # noqa: F401
    from rebvio_amd import backend as B
    from rebvio_amd import synth
    frames, cam = synth.render_stream(640, 480, 24)
    ctx = B.Context(B.default_params(480, 640, fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=15000, keylines_max=16000))
    maps = [ctx.detect_u8(frames[i], k * 50000) for k, i in enumerate(synth.pingpong_indices(24, 10))]
    for k in range(2):
        ctx.track_pair(maps[k], maps[k + 1])
    maps[2].mark_keyframe()
    snap = maps[2].keyframe_snapshot()  # at the mark, before the map serves as an old map
    for k in range(2, 9):
        ctx.track_pair(maps[k], maps[k + 1])
    time_pair(B, ctx, snap, maps[9], args.reps, "640x480 bench stream: the keyframe's snapshot and the map 7 pairs behind it, default filter")
    snap.release()
    ctx.close()
    small, qcam = synth.render_stream(576, 475, 2)
    big = np.ascontiguousarray(np.kron(small, np.ones((1, 4, 4), np.uint8)))
    H, W = big.shape[1:]
    ctx = B.Context(B.default_params(H, W, fm=qcam.fm * 4, cx=qcam.cx * 4 + 1.5, cy=qcam.cy * 4 + 1.5, keylines_ref=60000, keylines_max=65536))
    m = max((ctx.detect_u8(big[i], i * 50000) for i in range(2)), key=lambda x: x.size())
    kl = m.keylines()
    rng = np.random.default_rng(1)
    kl["matches"] = rng.integers(0, 6, len(kl))
    kl["rho"] = np.exp(rng.uniform(np.log(2e-3), np.log(15.0), len(kl))).astype(np.float32)
    kl["sigma_rho"] = (kl["rho"] * rng.uniform(0.0, 1.0, len(kl)).astype(np.float32)).astype(np.float32)
    m.upload(kl)
    snap = m.keyframe_snapshot()
    time_pair(B, ctx, snap, m, args.reps, f"{W}x{H}, keylines_max 65536, random depth state: a map and the snapshot taken from it, default filter")
    snap.release()
    ctx.close()


def host(args):
    from rebvio_amd import synth
    n = args.frames
    frames, cam = synth.render_stream(640, 480, 24)
    d = tempfile.mkdtemp()
    frames[synth.pingpong_indices(24, n)].tofile(os.path.join(d, "f.u8"))
    ts, gyro, acc = synth.imu_samples(synth.make_scene(0), n, noise_seed=1)
    rec = np.zeros(len(ts), dtype=[("ts", "<i8"), ("gyro", "<f4", 3), ("acc", "<f4", 3)])
    rec["ts"], rec["gyro"], rec["acc"] = ts, gyro * 0, acc
    rec.tofile(os.path.join(d, "imu.bin"))
    exe = os.path.join(ROOT, "rebvio_amd", "_build", "rebvio_replay")
    base = [exe, "--raw", os.path.join(d, "f.u8"), "--size", "640", "480", "--imu", os.path.join(d, "imu.bin"), "--camera", str(cam.fm),
            str(cam.cx), str(cam.cy), "--keylines", "15000", "16000", "--out", os.path.join(d, "o.txt"), "--kf-every", "10", "--kf-fuse",
            os.path.join(d, "fuse.txt")]
    rates = {"fuse": [], "fuse_cloud": []}
    clouds = points = 0
    for _ in range(args.rounds):
        for kind in ("fuse", "fuse_cloud"):
            r = subprocess.run(base + (["--kf-cloud", os.path.join(d, "kf_")] if kind == "fuse_cloud" else []), capture_output=True, text=True,
                               timeout=300)
            m = re.search(r"= (\d+) frames/s", r.stderr)
            if r.returncode != 0 or not m:
                print(json.dumps(dict(what="host class", kind=kind, rc=r.returncode, stderr=r.stderr[-400:])), flush=True)
                return
            rates[kind].append(int(m.group(1)))
            mp = re.search(r"kf_clouds=(\d+) kf_points=(\d+)", r.stderr)
            if mp:
                clouds, points = int(mp.group(1)), int(mp.group(2))
    med = {k: float(np.median(v)) for k, v in rates.items()}
    print(json.dumps(dict(what="rebvio::Rebvio on the 640x480 bench stream (rebvio_replay --kf-every 10 --kf-fuse), frames/s first to last record",
                          frames=n, without_kf_cloud=rates["fuse"], with_kf_cloud=rates["fuse_cloud"], median_without=med["fuse"],
                          median_with=med["fuse_cloud"], ratio=round(med["fuse_cloud"] / med["fuse"], 4), kf_clouds=clouds,
                          points_per_cloud=points // max(clouds, 1))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernels", "host"])
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    if "kernels" in a.what:
        kernels(a)
    if "host" in a.what:
        host(a)
