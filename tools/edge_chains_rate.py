#!/usr/bin/env python3
"""What the edge chains and polylines of a map cost. One JSON line per measurement on stdout.

  kernels   device time per launch of every k_chain_* / k_poly_* kernel (rebvio_hip_profile_*: HIP events around every launch) and
            the wall time of the synchronous calls rebvio_hip_map_edge_chains / rebvio_hip_map_edge_polylines, next to two
            yardsticks timed in the same process: k_join_edges (the kernel that writes the links) and the map's point-cloud
            extraction (k_cloud_count + k_cloud_emit + k_cloud_copy, rebvio_hip_map_point_cloud). `--reps` calls per round, three
            rounds, median and spread. On a tracked map of the 640x480 bench stream (about 16 000 keylines) and on a detected
            65 536-keyline map with depths planted.

  host      rebvio::Rebvio (rebvio_replay) on `--frames` frames of the bench stream: plain, with --cloud and with --polylines,
            processes alternating, `--rounds` times each

    tools/edge_chains_rate.py [kernels] [host] [--reps K] [--frames N] [--rounds R]"""
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
CHAIN = ("k_chain_link", "k_chain_round", "k_chain_rank", "k_chain_count", "k_chain_emit", "k_chain_order")
POLY = ("k_poly_count", "k_poly_emit", "k_poly_lines")
CLOUD = ("k_cloud_count", "k_cloud_emit", "k_cloud_copy")


def wall(call, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    return round((time.perf_counter() - t0) / reps * 1e6, 1)


def profiled(ctx, call, reps, names, only):
    """{kernel: (mean device us per launch, launches per call)} over reps calls"""
    ctx.profile(True, only=only)
    ctx.profile_reset()
    for _ in range(reps):
        call()
    prof = ctx.profile_read()
    ctx.profile(False)
    return {k: (round(prof[k][0], 2), prof[k][1] / reps) for k in names if k in prof}


def time_map(B, ctx, m, frame, reps, what):
    refs, order, starts, nk, nc = m.edge_chains()      # warm: scratch allocated
    pts, refs2, lines, npts, nl = m.edge_polylines()
    cloud = m.point_cloud()
    lengths = np.diff(starts)
    out = dict(what=what, keylines=nk, chains=nc, longest=int(lengths.max()) if nc else 0, chains_of_8_or_more=int((lengths >= 8).sum()),
               cyclic=int((refs["flags"][refs["rank"] == 0] & 1).sum()), polyline_points=npts, polylines=nl, cloud_points=len(cloud), reps=reps,
               rounds_launched=int(np.ceil(np.log2(ctx.p.keylines_max))))
    rows = {}
    for _ in range(3):
        for key, call, names, only in (("chains", m.edge_chains, CHAIN, "k_chain_*"), ("polylines", m.edge_polylines, CHAIN + POLY, "k_*"),
                                       ("cloud", m.point_cloud, CLOUD, "k_cloud_*"),
                                       ("detect", lambda: ctx.detect_u8(frame, 0).release(), ("k_join_edges",), "k_join_edges")):
            prof = profiled(ctx, call, reps if key != "detect" else max(1, reps // 10), names, only)
            for k, (us, per_call) in prof.items():
                rows.setdefault(f"{key}:{k}", []).append((us, per_call))
        # device time of one call = sum over kernels of (mean per launch x launches per call)
        for key in ("chains", "polylines", "cloud"):
            tot = sum(v[-1][0] * v[-1][1] for k, v in rows.items() if k.startswith(key + ":k_"))
            rows.setdefault(f"{key}:device_us_per_call", []).append((round(tot, 2), 1))
        for key, call in (("chains", m.edge_chains), ("polylines", m.edge_polylines), ("cloud", m.point_cloud)):
            rows.setdefault(f"{key}:call_wall_us", []).append((wall(call, reps), 1))
        # the chain entry without its downloads: counts only
        rows.setdefault("chains:call_wall_us_counts_only", []).append((wall(lambda: m.edge_chains(cap_keylines=0, cap_chains=0), reps), 1))
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
    time_map(B, ctx, maps[9], frames[idx[9]], args.reps, "640x480 bench stream, the new map of the ninth pair")
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
    time_map(B, ctx, m, frame, args.reps, "896x640 noise frame, keylines_max 65536, detection's own links, depths planted")
    perm = rng.permutation(len(kl))
    kl["id_prev"], kl["id_next"] = -1, -1
    kl["id_next"][perm[:-1]], kl["id_prev"][perm[1:]] = perm[1:], perm[:-1]
    m.upload(kl)
    time_map(B, ctx, m, frame, args.reps, "the same map, its links one path in shuffled index order: every round works")
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
    rates = {"plain": [], "cloud": [], "polylines": []}
    extra = {"plain": [], "cloud": ["--cloud", os.path.join(d, "c_")], "polylines": ["--polylines", os.path.join(d, "p_")]}
    counts = ""
    for _ in range(args.rounds):
        for kind in rates:
            r = subprocess.run(base + extra[kind], capture_output=True, text=True, timeout=900)
            m = re.search(r"= (\d+) frames/s", r.stderr)
            if r.returncode != 0 or not m:
                print(json.dumps(dict(what="host class", kind=kind, rc=r.returncode, stderr=r.stderr[-400:])), flush=True)
                return
            rates[kind].append(int(m.group(1)))
            if kind == "polylines":
                counts = re.search(r"polyline_files=.*", r.stderr).group(0)
            for f in os.listdir(d):  # a run's PLY files go before the next run writes its own
                if f.endswith(".ply"):
                    os.remove(os.path.join(d, f))
    shutil.rmtree(d, ignore_errors=True)
    med = {k: float(np.median(v)) for k, v in rates.items()}
    print(json.dumps(dict(what="rebvio::Rebvio on the 640x480 bench stream (rebvio_replay), frames/s first to last record; --cloud and "
                               "--polylines write one PLY file per record", frames=n, plain=rates["plain"], with_cloud=rates["cloud"],
                          with_polylines=rates["polylines"], median_plain=med["plain"], median_cloud=med["cloud"],
                          median_polylines=med["polylines"], polylines_over_plain=round(med["polylines"] / med["plain"], 4),
                          polylines_over_cloud=round(med["polylines"] / med["cloud"], 4), last_polylines_run=counts)), flush=True)


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
