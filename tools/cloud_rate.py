#!/usr/bin/env python3
"""What the point cloud costs.  One JSON line per measurement on stdout.

  kernels   device time of k_cloud_count / k_cloud_emit / k_cloud_copy (rebvio_hip_profile_*: HIP events around every launch) and the wall time of
            a synchronous rebvio_hip_map_point_cloud call, on a tracked map of the 640x480 bench stream (~15 k keylines) and on a
            65 536-keyline map, next to the compulsory bytes: 24 B read per keyline + 32 B written per point
  host      rebvio::Rebvio (rebvio_replay) on the bench stream without and with a registered point-cloud callback (--cloud-dry: no
            files), alternating, `--rounds` times each; the callback's price as the ratio of the median rates

    tools/cloud_rate.py [kernels] [host] [--frames N] [--rounds R] [--reps K]"""
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


def crafted(kl, seed):
    rng = np.random.default_rng(seed)
    kl = kl.copy()
    n = len(kl)
    kl["matches"] = rng.integers(0, 6, n)
    kl["rho"] = np.exp(rng.uniform(np.log(2e-3), np.log(15.0), n)).astype(np.float32)
    kl["sigma_rho"] = (kl["rho"] * rng.uniform(0.0, 1.0, n).astype(np.float32)).astype(np.float32)
    return kl


def time_map(B, ctx, m, reps, what):
    n = m.size()
    flt = B.default_cloud_filter()
    pts, count = m.point_cloud(flt, return_count=True)  # warm: buffers allocated
    ctx.profile(True, only="k_cloud*")
    ctx.profile_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        m.point_cloud(flt, cap=n)
    wall = (time.perf_counter() - t0) / reps * 1e6
    prof = ctx.profile_read()
    ctx.profile(False)
    t_count, t_emit, t_copy = prof["k_cloud_count"][0], prof["k_cloud_emit"][0], prof["k_cloud_copy"][0]
    nbytes = 24 * n + 32 * count
    print(json.dumps(dict(what=what, keylines=n, points=count, share=round(count / n, 4), reps=reps,
                          k_cloud_count_us=round(t_count, 2), k_cloud_emit_us=round(t_emit, 2), k_cloud_copy_us=round(t_copy, 2),
                          copy_bytes=32 * count, copy_GBps=round(32 * count / (t_copy * 1e-6) / 1e9, 2),
                          sync_call_wall_us=round(wall, 1), compulsory_bytes=nbytes,
                          emit_GBps=round((24 * n + 32 * count) / (t_emit * 1e-6) / 1e9, 2),
                          count_GBps=round(12 * n / (t_count * 1e-6) / 1e9, 2))), flush=True)


def kernels(args):
    import torch  # noqa: F401
    from rebvio_amd import backend as B
    from rebvio_amd import synth
    frames, cam = synth.render_stream(640, 480, 8)
    ctx = B.Context(B.default_params(480, 640, fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=15000, keylines_max=16000))
    maps = [ctx.detect_u8(frames[i], i * 50000) for i in range(8)]
    for k in range(7):
        ctx.track_pair(maps[k], maps[k + 1])
    time_map(B, ctx, maps[-1], args.reps, "640x480 bench stream, map after 7 pairs, default filter")
    ctx.close()
    small, qcam = synth.render_stream(576, 475, 2)
    big = np.ascontiguousarray(np.kron(small, np.ones((1, 4, 4), np.uint8)))
    H, W = big.shape[1:]
    ctx = B.Context(B.default_params(H, W, fm=qcam.fm * 4, cx=qcam.cx * 4 + 1.5, cy=qcam.cy * 4 + 1.5, keylines_ref=60000, keylines_max=65536))
    m = max((ctx.detect_u8(big[i], i * 50000) for i in range(2)), key=lambda x: x.size())
    m.upload(crafted(m.keylines(), 1))
    time_map(B, ctx, m, args.reps, f"{W}x{H}, keylines_max 65536, random depth state, default filter")
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
            str(cam.cx), str(cam.cy), "--keylines", "15000", "16000", "--out", os.path.join(d, "o.txt")]
    rates = {"plain": [], "cloud": []}
    points = 0
    for _ in range(args.rounds):
        for kind in ("plain", "cloud"):
            r = subprocess.run(base + (["--cloud-dry"] if kind == "cloud" else []), capture_output=True, text=True, timeout=300)
            m = re.search(r"= (\d+) frames/s", r.stderr)
            if r.returncode != 0 or not m:
                print(json.dumps(dict(what="host class", kind=kind, rc=r.returncode, stderr=r.stderr[-400:])), flush=True)
                return
            rates[kind].append(int(m.group(1)))
            mp = re.search(r"clouds=(\d+) points=(\d+)", r.stderr)
            if mp:
                points = int(mp.group(2)) // max(int(mp.group(1)), 1)
    med = {k: float(np.median(v)) for k, v in rates.items()}
    print(json.dumps(dict(what="rebvio::Rebvio on the 640x480 bench stream (rebvio_replay), frames/s first to last record", frames=n,
                          plain=rates["plain"], with_cloud_callback=rates["cloud"], median_plain=med["plain"], median_cloud=med["cloud"],
                          ratio=round(med["cloud"] / med["plain"], 4), points_per_cloud=points)), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernels", "host"])
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=300)
    a = ap.parse_args()
    if "kernels" in a.what:
        kernels(a)
    if "host" in a.what:
        host(a)
