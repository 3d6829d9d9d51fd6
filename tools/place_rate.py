#!/usr/bin/env python3
"""What place recognition costs. One JSON line per measurement on stdout.

Device time per launch of k_place_hist, k_place_norm, k_place_dist and k_place_topk (rebvio_hip_profile_*: a HIP event pair around
every launch, the method of DESIGN.md 5n) and the wall time of the entries: the signature of a tracked map of the 640x480 bench
stream (about 15 000 keylines) and of an empty map of the same context (an empty launch of the same grid), and queries from a
signature against databases of 256, 4096 and 65 536 random rows with k = 4 and k = 16. For k_place_dist the achieved bandwidth is the
rows' bytes (768 per row) over the kernel's time. `--reps` calls per round, three rounds, median and spread.

    tools/place_rate.py [--reps K]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("k_place_hist", "k_place_norm", "k_place_dist", "k_place_topk")


def wall(call, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    return round((time.perf_counter() - t0) / reps * 1e6, 1)


def profiled(ctx, call, reps):
    """mean device us per launch of every place kernel over reps calls"""
    out = {}
    for name in KERNELS:
        ctx.profile(True, only=name)
        ctx.profile_reset()
        for _ in range(reps):
            call()
        prof = ctx.profile_read()
        ctx.profile(False)
        if name in prof and prof[name][1]:
            out[name] = round(prof[name][0], 2)
    return out


def measure(ctx, call, reps, out):
    rows = {}
    for _ in range(3):
        for name, us in profiled(ctx, call, reps).items():
            rows.setdefault(name, []).append(us)
        rows.setdefault("call_wall_us", []).append(wall(call, reps))
    for k, v in rows.items():
        out[k] = dict(median_us=float(np.median(v)), spread_us=round(max(v) - min(v), 2), rounds=v)
    return out


def main(args):
    import torch  # noqa: F401
    from rebvio_amd import backend as B
    from rebvio_amd import synth
    frames, cam = synth.render_stream(640, 480, 10)
    kw = dict(fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=15000, keylines_max=16000)
    ctx = B.Context(B.default_params(480, 640, **kw))
    maps = [ctx.detect_u8(frames[k], k * 50000) for k in range(10)]
    for k in range(9):
        ctx.track_pair(maps[k], maps[k + 1])
    empty = ctx.detect_u8(np.full((480, 640), 128, np.uint8), 500000)
    assert empty.size() == 0
    m = maps[9]
    sig, counted = m.place_signature()
    for what, mm in (("640x480 bench stream, the new map of the ninth pair", m), ("an empty map of the same context", empty)):
        out = dict(what="signature: " + what, keylines=mm.size(), counted=mm.place_signature()[1], reps=args.reps)
        print(json.dumps(measure(ctx, lambda: mm.place_signature(), args.reps, out)), flush=True)
    rng = np.random.default_rng(7)
    for size in (256, 4096, 65536):
        db = ctx.place_db(size)
        rows = rng.integers(0, 65536, (size, 384), dtype=np.uint16)
        for r in rows:
            db.add_signature(r)
        for k in (4, 16):
            out = dict(what=f"query from a signature, {size} random rows, k = {k}", rows=size, k=k, bytes=size * 768, reps=args.reps)
            measure(ctx, lambda: db.query_signature(sig, k), args.reps, out)
            out["k_place_dist_GBps"] = round(size * 768 / (out["k_place_dist"]["median_us"] * 1e-6) / 1e9, 1)
            print(json.dumps(out), flush=True)
        out = dict(what=f"query from the map, {size} random rows, k = 4", rows=size, k=4, reps=args.reps)
        print(json.dumps(measure(ctx, lambda: db.query(m, 4), args.reps, out)), flush=True)
        db.release()
    ctx.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    main(ap.parse_args())
