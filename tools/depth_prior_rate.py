#!/usr/bin/env python3
"""What fusing a registered depth image into a map costs. One JSON line per measurement on stdout.

  kernels   device time per launch of k_depth_prior (rebvio_hip_profile_*: a HIP event pair around every launch, the method of
            DESIGN.md 5n) next to two yardsticks timed in the same process: the same launch over an EMPTY map of the same context
            (every thread falls through: an empty launch of this grid) and the map's point-cloud extraction (k_cloud_count,
            k_cloud_emit). A figure at the empty launch's says no more than "an empty launch". Then the wall time of the three
            entries: host image, device image, queued (the call alone, and with rebvio_hip_depth_prior_last_counts behind it).
            `--reps` calls per round, three rounds, median and spread. On a tracked map of the 640x480 bench stream (about 15 000
            keylines, rendered depth) and on a detected 65 536-keyline map (896x640 noise frame, random depth).

  host      rebvio::Rebvio (rebvio_replay) on `--frames` frames of the bench stream: plain and with --depth, processes alternating,
            `--rounds` times each

    tools/depth_prior_rate.py [kernels] [host] [--reps K] [--frames N] [--rounds R]"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLOUD = ("k_cloud_count", "k_cloud_emit")


def wall(call, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    return round((time.perf_counter() - t0) / reps * 1e6, 1)


def profiled(ctx, call, reps, names, only):
    """{kernel: mean device us per launch} over reps calls"""
    ctx.profile(True, only=only)
    ctx.profile_reset()
    for _ in range(reps):
        call()
    prof = ctx.profile_read()
    ctx.profile(False)
    return {k: round(prof[k][0], 2) for k in names if k in prof}


def time_map(B, ctx, m, m_empty, depth, reps, what):
    fmt = B.DEPTH_U16 if depth.dtype == np.uint16 else B.DEPTH_F32
    dev = ctx.upload_bytes(depth)
    counts = m.fuse_depth_image(dev, fmt, device=True)     # warm: scratch allocated
    m.fuse_depth_image(depth)                              # ... and the host entry's staging frame
    m.point_cloud()
    out = dict(what=what, keylines=counts.candidates, counts=counts.as_tuple(), format="u16" if fmt == B.DEPTH_U16 else "f32", reps=reps)
    rows = {}
    for _ in range(3):
        for key, call, names, only in (("fuse", lambda: m.fuse_depth_image(dev, fmt, device=True), ("k_depth_prior",), "k_depth_prior"),
                                       ("empty", lambda: m_empty.fuse_depth_image(dev, fmt, device=True), ("k_depth_prior",), "k_depth_prior"),
                                       ("cloud", m.point_cloud, CLOUD, "k_cloud_*")):
            for k, us in profiled(ctx, call, reps, names, only).items():
                rows.setdefault(f"{key}:{k}", []).append(us)

        def queued():
            m.fuse_depth_image(dev, fmt, queued=True)

        def queued_and_counts():
            m.fuse_depth_image(dev, fmt, queued=True)
            ctx.depth_prior_last_counts()
        for key, call in (("host_entry", lambda: m.fuse_depth_image(depth)), ("device_entry", lambda: m.fuse_depth_image(dev, fmt, device=True)),
                          ("queued_entry_and_last_counts", queued_and_counts), ("cloud_call", m.point_cloud)):
            rows.setdefault(f"{key}:call_wall_us", []).append(wall(call, reps))
        rows.setdefault("queued_entry:call_wall_us", []).append(wall(queued, reps))
        ctx.depth_prior_last_counts()  # (drains the queue before the next round)
    for k, v in rows.items():
        out[k] = dict(median_us=float(np.median(v)), spread_us=round(max(v) - min(v), 2), rounds=v)
    print(json.dumps(out), flush=True)


def kernels(args):
    import torch  # noqa: F401
    from rebvio_amd import backend as B
    from rebvio_amd import synth
    frames, cam = synth.render_stream(640, 480, 24)
    ctx = B.Context(B.default_params(480, 640, fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=15000, keylines_max=16000))
    idx = synth.pingpong_indices(24, 10)
    maps = [ctx.detect_u8(frames[i], k * 50000) for k, i in enumerate(idx)]
    for k in range(9):
        ctx.track_pair(maps[k], maps[k + 1])
    empty = ctx.detect_u8(np.full((480, 640), 128, np.uint8), 500000)
    assert empty.size() == 0
    depth = synth.render_depth(synth.make_scene(0), cam, float(idx[9]))
    time_map(B, ctx, maps[9], empty, np.rint(depth.astype(np.float64) * 1000).astype(np.uint16), args.reps,
             "640x480 bench stream, the new map of the ninth pair, rendered depth as u16 millimetres")
    time_map(B, ctx, maps[9], empty, depth, args.reps, "the same map, the depth as f32 metres")
    ctx.close()
    rng = np.random.default_rng(3)
    frame = rng.integers(0, 256, (640, 896)).astype(np.uint8)
    ctx = B.Context(B.default_params(640, 896, fm=500.0, cx=447.5, cy=319.5, keylines_ref=60000, keylines_max=65536))
    m = ctx.detect_u8(frame, 0)
    empty = ctx.detect_u8(np.full((640, 896), 128, np.uint8), 50000)
    assert empty.size() == 0
    time_map(B, ctx, m, empty, rng.integers(500, 12000, (640, 896)).astype(np.uint16), args.reps,
             "896x640 noise frame, keylines_max 65536, random u16 depth: every tap gathers from another line")
    ctx.close()


def host(args):
    from rebvio_amd import synth
    n = args.frames
    frames, cam = synth.render_stream(640, 480, 24)
    depth = np.rint(synth.render_stream_depth(640, 480, 24).astype(np.float64) * 1000).astype("<u2")
    d = tempfile.mkdtemp()
    idx = synth.pingpong_indices(24, n)
    frames[idx].tofile(os.path.join(d, "f.u8"))
    depth[idx].tofile(os.path.join(d, "d.u16"))
    ts, gyro, acc = synth.imu_samples(synth.make_scene(0), n, noise_seed=1)
    rec = np.zeros(len(ts), dtype=[("ts", "<i8"), ("gyro", "<f4", 3), ("acc", "<f4", 3)])
    rec["ts"], rec["gyro"], rec["acc"] = ts, gyro * 0, acc
    rec.tofile(os.path.join(d, "imu.bin"))
    exe = os.path.join(ROOT, "rebvio_amd", "_build", "rebvio_replay")
    base = [exe, "--raw", os.path.join(d, "f.u8"), "--size", "640", "480", "--imu", os.path.join(d, "imu.bin"), "--camera", str(cam.fm),
            str(cam.cx), str(cam.cy), "--keylines", "15000", "16000", "--out", os.path.join(d, "o.txt")]
    rates = {"plain": [], "depth": []}
    extra = {"plain": [], "depth": ["--depth", os.path.join(d, "d.u16")]}
    counts = ""
    for _ in range(args.rounds):
        for kind in rates:
            r = subprocess.run(base + extra[kind], capture_output=True, text=True, timeout=900)
            m = re.search(r"= (\d+) frames/s", r.stderr)
            if r.returncode != 0 or not m:
                print(json.dumps(dict(what="host class", kind=kind, rc=r.returncode, stderr=r.stderr[-400:])), flush=True)
                return
            rates[kind].append(int(m.group(1)))
            if kind == "depth":
                counts = re.search(r"depth_images=.*", r.stderr).group(0)
    shutil.rmtree(d, ignore_errors=True)
    med = {k: float(np.median(v)) for k, v in rates.items()}
    print(json.dumps(dict(what="rebvio::Rebvio on the 640x480 bench stream (rebvio_replay), frames/s first to last record; --depth reads, "
                               "copies, uploads and fuses one u16 image per frame and keeps the reader seven frames ahead at most",
                          frames=n, plain=rates["plain"], with_depth=rates["depth"], median_plain=med["plain"], median_depth=med["depth"],
                          depth_over_plain=round(med["depth"] / med["plain"], 4), last_depth_run=counts)), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernels", "host"])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if "kernels" in a.what:
        kernels(a)
    if "host" in a.what:
        host(a)
