#!/usr/bin/env python3
"""What fusing a rectified stereo partner's edge map into a map costs. One JSON line per measurement on stdout.

Device time per launch of k_stereo_prior (rebvio_hip_profile_*: a HIP event pair around every launch, the method of DESIGN.md 5n)
next to two yardsticks timed in the same process: the same launch over an EMPTY left map of the same context (every sub-group falls
through: an empty launch of this grid) and k_depth_prior on the same map (one thread per keyline, three gathered taps). A figure at
the empty launch's says no more than "an empty launch". Then the wall time of the entries: synchronous, queued (the call alone, and
with rebvio_hip_stereo_prior_last_counts behind it). `--reps` calls per round, three rounds, median and spread. On a tracked map of
the 640x480 bench stereo stream (about 15 000 keylines; the right map from a second context) and on a detected 65 536-keyline pair
of maps (896x640 noise frames).

    tools/stereo_prior_rate.py [--reps K]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BASELINE = 0.2


def wall(call, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    return round((time.perf_counter() - t0) / reps * 1e6, 1)


def profiled(ctx, call, reps, name):
    """mean device us per launch of kernel `name` over reps calls"""
    ctx.profile(True, only=name)
    ctx.profile_reset()
    for _ in range(reps):
        call()
    prof = ctx.profile_read()
    ctx.profile(False)
    return round(prof[name][0], 2)


def time_maps(B, ctx, m, mr, m_empty, depth, opts, reps, what):
    # (repeated launches tighten the same keylines; the windows walked and the keylines gathered are the same every time)
    dev = ctx.upload_bytes(depth)
    counts = m.fuse_stereo(mr, opts)                      # warm: scratch allocated
    m.fuse_depth_image(dev, B.DEPTH_F32, device=True)
    out = dict(what=what, keylines=counts.candidates, right_keylines=mr.size(), counts=counts.as_tuple(), d_max=opts.d_max, reps=reps)
    rows = {}
    for _ in range(3):
        for key, call, name in (("fuse", lambda: m.fuse_stereo(mr, opts), "k_stereo_prior"),
                                ("empty", lambda: m_empty.fuse_stereo(mr, opts), "k_stereo_prior"),
                                ("depth_prior", lambda: m.fuse_depth_image(dev, B.DEPTH_F32, device=True), "k_depth_prior")):
            rows.setdefault(f"{key}:{name}", []).append(profiled(ctx, call, reps, name))

        def queued():
            m.fuse_stereo(mr, opts, queued=True)

        def queued_and_counts():
            m.fuse_stereo(mr, opts, queued=True)
            ctx.stereo_prior_last_counts()
        for key, call in (("sync_entry", lambda: m.fuse_stereo(mr, opts)), ("queued_entry_and_last_counts", queued_and_counts)):
            rows.setdefault(f"{key}:call_wall_us", []).append(wall(call, reps))
        rows.setdefault("queued_entry:call_wall_us", []).append(wall(queued, reps))
        ctx.stereo_prior_last_counts()  # (drains the queue before the next round)
    for k, v in rows.items():
        out[k] = dict(median_us=float(np.median(v)), spread_us=round(max(v) - min(v), 2), rounds=v)
    print(json.dumps(out), flush=True)


def main(args):
    import torch  # noqa: F401
    from rebvio_amd import backend as B
    from rebvio_amd import synth
    left, right, cam = synth.render_stereo_stream(640, 480, 10, BASELINE)
    kw = dict(fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=15000, keylines_max=16000)
    ctx, rctx = B.Context(B.default_params(480, 640, **kw)), B.Context(B.default_params(480, 640, **kw))
    maps = [ctx.detect_u8(left[k], k * 50000) for k in range(10)]
    rmaps = [rctx.detect_u8(right[k], k * 50000) for k in range(10)]
    o = B.default_stereo_prior_opts(ctx, baseline=BASELINE)
    maps[0].fuse_stereo(rmaps[0], o)
    for k in range(9):
        ctx.track_pair(maps[k], maps[k + 1])
        if k < 8:
            maps[k + 1].fuse_stereo(rmaps[k + 1], o)
    empty = ctx.detect_u8(np.full((480, 640), 128, np.uint8), 500000)
    assert empty.size() == 0
    depth = synth.render_depth(synth.make_scene(0), cam, 9.0)
    time_maps(B, ctx, maps[9], rmaps[9], empty, depth, o, args.reps,
              "640x480 bench stereo stream, baseline 0.2 m, the new map of the ninth pair against the right map of its frame (a second context)")
    ctx.close()
    rctx.close()
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (2, 640, 896)).astype(np.uint8)
    ctx = B.Context(B.default_params(640, 896, fm=500.0, cx=447.5, cy=319.5, keylines_ref=60000, keylines_max=65536))
    m, mr = ctx.detect_u8(frames[0], 0), ctx.detect_u8(frames[1], 50000)
    empty = ctx.detect_u8(np.full((640, 896), 128, np.uint8), 100000)
    assert empty.size() == 0
    time_maps(B, ctx, m, mr, empty, rng.uniform(0.5, 12.0, (640, 896)).astype(np.float32), B.default_stereo_prior_opts(ctx, baseline=BASELINE),
              args.reps, "896x640 noise frames, keylines_max 65536, both maps of one context: every window is full of keylines to gather")
    ctx.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    main(ap.parse_args())
