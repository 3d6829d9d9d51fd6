#!/usr/bin/env python3
"""What the straight segments of a map cost. One JSON line per measurement on stdout.

  kernels   device time per launch of every k_seg_* kernel (rebvio_hip_profile_*: HIP events around every launch) and the wall
            time of the synchronous call rebvio_hip_map_edge_segments beside rebvio_hip_map_edge_polylines on the same map in the
            same process; rounds_used, segments kept, bytes downloaded against the polylines' bytes. `--reps` calls per round,
            three rounds, median and spread. On a tracked map of the 640x480 bench stream (the ninth pair's new map) and on a
            detected 65 536-keyline noise map with depths planted.

  host      rebvio::Rebvio (rebvio_replay) on `--frames` frames of the bench stream: plain, with --polylines and with --segments,
            processes alternating, `--rounds` times each

    tools/edge_segments_rate.py [kernels] [host] [--reps K] [--frames N] [--rounds R]"""
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
SEG = ("k_seg_init", "k_seg_far", "k_seg_split", "k_seg_count", "k_seg_emit", "k_seg_fit")


def wall(call, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    return round((time.perf_counter() - t0) / reps * 1e6, 1)


def profiled(ctx, call, reps):
    """{kernel: (mean device us per launch, launches per call)} over reps calls, and the launches of one call"""
    ctx.profile(True, only="k_*")
    ctx.profile_reset()
    for _ in range(reps):
        call()
    prof = ctx.profile_read()
    ctx.profile(False)
    return {k: (round(v[0], 2), v[1] / reps) for k, v in prof.items() if v[1]}


def time_map(B, ctx, m, reps, what):
    segs, cnt = m.edge_segments()      # warm: scratch allocated
    pts, refs2, lines, npts, nl = m.edge_polylines()
    out = dict(what=what, keylines=m.size(), reps=reps, counts=cnt.as_dict(),
               points_in_kept_segments=int(segs["points"].sum()), median_points_per_segment=float(np.median(segs["points"])) if len(segs) else 0.0,
               segment_bytes=int(segs.nbytes), polyline_bytes=int(pts.nbytes + refs2.nbytes + lines.nbytes))
    rows = {}
    for _ in range(3):
        prof = profiled(ctx, m.edge_segments, reps)
        for k, (us, per_call) in prof.items():
            rows.setdefault(f"segments:{k}", []).append((us, per_call))
        rows.setdefault("segments:launches_per_call", []).append((sum(v[1] for v in prof.values()), 1))
        rows.setdefault("segments:device_us_per_call", []).append((round(sum(us * n for us, n in prof.values()), 2), 1))
        rows.setdefault("segments:device_us_per_call_k_seg_only", []).append((round(sum(us * n for k, (us, n) in prof.items() if k in SEG), 2), 1))
        rows.setdefault("segments:call_wall_us", []).append((wall(m.edge_segments, reps), 1))
        rows.setdefault("polylines:call_wall_us", []).append((wall(m.edge_polylines, reps), 1))
        rows.setdefault("segments:call_wall_us_counts_only", []).append((wall(lambda: m.edge_segments(cap=0), reps), 1))
    for k, v in rows.items():
        us = [x[0] for x in v]
        out[k] = dict(median_us=float(np.median(us)), spread_us=round(max(us) - min(us), 2), launches_per_call=v[0][1], rounds=us)
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
    time_map(B, ctx, maps[9], args.reps, "640x480 bench stream, the new map of the ninth pair, default options")
    # the geometry alone: every keyline kept (the wide filter), the rounds the default max_rounds rests on
    wide = B.default_segment_opts(max_rounds=32, poly=dict(filter=dict(min_matches=0, max_rel_sigma=1e9)))
    for tol in (1.0, 0.7):
        wide.tol = tol
        segs, cnt = maps[9].edge_segments(wide)
        print(json.dumps(dict(what="the same map, every keyline kept, max_rounds 32", tol=tol, counts=cnt.as_dict(),
                              points_in_kept_segments=int(segs["points"].sum()), median_points_per_segment=float(np.median(segs["points"])))), flush=True)
    ctx.close()
    frame = np.random.default_rng(3).integers(0, 256, (640, 896)).astype(np.uint8)
    ctx = B.Context(B.default_params(640, 896, fm=500.0, cx=447.5, cy=319.5, keylines_ref=60000, keylines_max=65536))
    m = ctx.detect_u8(frame, 0)
    kl = m.keylines()
    rng = np.random.default_rng(1)
    kl["matches"] = 3
    kl["rho"] = rng.uniform(0.2, 2.0, len(kl)).astype(np.float32)
    kl["sigma_rho"] = (0.05 * kl["rho"]).astype(np.float32)
    m.upload(kl)
    time_map(B, ctx, m, args.reps, "896x640 noise frame, keylines_max 65536, detection's own links, depths planted")
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
    rates = {"plain": [], "polylines": [], "segments": []}
    extra = {"plain": [], "polylines": ["--polylines", os.path.join(d, "p_")], "segments": ["--segments", os.path.join(d, "s_")]}
    counts, sizes = {}, {}
    for _ in range(args.rounds):
        for kind in rates:
            r = subprocess.run(base + extra[kind], capture_output=True, text=True, timeout=900)
            m = re.search(r"= (\d+) frames/s", r.stderr)
            if r.returncode != 0 or not m:
                print(json.dumps(dict(what="host class", kind=kind, rc=r.returncode, stderr=r.stderr[-400:])), flush=True)
                return
            rates[kind].append(int(m.group(1)))
            c = re.search(r"(polyline|segment)_files=.*", r.stderr)
            if c:
                counts[kind] = c.group(0)
            ply = [f for f in os.listdir(d) if f.endswith(".ply")]
            if ply:
                sizes[kind] = round(sum(os.path.getsize(os.path.join(d, f)) for f in ply) / len(ply))
            for f in ply:  # a run's PLY files go before the next run writes its own
                os.remove(os.path.join(d, f))
    shutil.rmtree(d, ignore_errors=True)
    med = {k: float(np.median(v)) for k, v in rates.items()}
    print(json.dumps(dict(what="rebvio::Rebvio on the 640x480 bench stream (rebvio_replay), frames/s first to last record; --polylines and "
                               "--segments write one PLY file per record", frames=n, rates=rates, median=med,
                          polylines_over_plain=round(med["polylines"] / med["plain"], 4), segments_over_plain=round(med["segments"] / med["plain"], 4),
                          mean_file_bytes=sizes, last_runs=counts)), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernels", "host"])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if "kernels" in a.what:
        kernels(a)
    if "host" in a.what:
        host(a)
