#!/usr/bin/env python3
"""Frames/s of the streaming driver for each camera pixel format (REBVIO_HIP_PX_*) against GRAY8, 640x480, in four setups:
one stream with device-resident frames, one stream with host frames (pinned ring + copy kernel), 8 lanes of a batch with
device-resident frames, one stream with a lens model (device frames, the front end's gather converts the taps).
  pixel_format_rate.py [steps] [warmup] [--formats GRAY8,RGB8,...] [--setups device,host,batch8,lens] [--repeat N]
Prints one JSON line per (setup, format) with the rate and its ratio to GRAY8 in the same setup (median of --repeat windows,
GRAY8 measured first and again last: the spread of the two is the run-to-run noise of the setup)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401
from rebvio_amd import backend as B, shard, synth  # noqa: E402

NAMES = ["GRAY8", "RGB8", "BGR8", "RGBA8", "BGRA8", "YUYV", "UYVY"]
EUROC_D = [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0]

ap = argparse.ArgumentParser()
ap.add_argument("steps", nargs="?", type=int, default=2000)
ap.add_argument("warmup", nargs="?", type=int, default=500)
ap.add_argument("--formats", default=",".join(NAMES))
ap.add_argument("--setups", default="device,host,batch8,lens")
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--no-bind", action="store_true")
a = ap.parse_args()

if not a.no_bind:  # like bench.py: the CPUs of the GPU's NUMA node
    _pr = torch.cuda.get_device_properties(0)
    shard.bind_to_gpu_numa_node(f"{_pr.pci_domain_id:04x}:{_pr.pci_bus_id:02x}:{_pr.pci_device_id:02x}.0")

W, H, NF = 640, 480, 24
cam = synth.Camera.for_size(W, H)
params = B.default_params(H, W, fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=15000, keylines_max=16000)


_grey = {}


def grey_stream(stream_id):
    if stream_id not in _grey:
        _grey[stream_id] = synth.render_stream(W, H, NF, stream_id=stream_id)[0]
    return _grey[stream_id]


def px_frames(grey, fmt):
    """colour frames whose grey is close to `grey` (chroma offsets); YUYV / UYVY carry grey as Y"""
    rng = np.random.default_rng(fmt)
    g = grey.astype(np.int16)
    if fmt == 0:
        return grey
    if fmt >= 5:
        c = rng.integers(0, 256, grey.shape, dtype=np.uint8)
        return np.stack([grey, c] if fmt == 5 else [c, grey], -1)
    rgb = np.clip(np.stack([g + rng.integers(-30, 31, g.shape, dtype=np.int16), g, g - 10], -1), 0, 255).astype(np.uint8)
    if fmt in (2, 4):
        rgb = rgb[..., ::-1]
    if fmt in (3, 4):
        rgb = np.concatenate([rgb, np.full(grey.shape + (1,), 255, np.uint8)], -1)
    return np.ascontiguousarray(rgb)


def window(push, k0, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(k0, k0 + n):
        push(k)
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def measure(setup, fmt):
    order = synth.pingpong_indices(NF, a.warmup + a.repeat * a.steps + 8)
    bpp = B.PX_BPP[fmt]
    if setup == "batch8":
        L = 8
        bat = B.Batch(params, L)
        devs = [bat.lanes[l].upload_frames(px_frames(grey_stream(l), fmt)) for l in range(L)]
        fb = W * H * bpp

        def push(k):
            bat.push_px_device([d + int(order[k]) * fb for d in devs], fmt, k * 50000)
    else:
        ctx = B.Context(params)
        if setup == "lens":
            ctx.set_undistort(cam.fm, cam.fm, cam.cx, cam.cy, EUROC_D)
        frames = px_frames(grey_stream(0), fmt)
        if setup == "host":
            def push(k):
                ctx.push_frame_px(frames[int(order[k])], fmt, k * 50000)
        else:
            dev = ctx.upload_frames(frames)
            fb = W * H * bpp

            def push(k):
                ctx.push_frame_px_device(dev + int(order[k]) * fb, fmt, k * 50000)
    window(push, 0, a.warmup)
    rates = [window(push, a.warmup + r * a.steps, a.steps) for r in range(a.repeat)]
    (bat if setup == "batch8" else ctx).flush()
    (bat if setup == "batch8" else ctx).close()
    return statistics.median(rates) * (8 if setup == "batch8" else 1), rates


fmts = [NAMES.index(f) for f in a.formats.split(",")]
for setup in a.setups.split(","):
    grey0, _ = measure(setup, 0)
    res = {}
    for fmt in fmts:
        if fmt == 0:
            continue
        res[fmt] = measure(setup, fmt)
    grey1, _ = measure(setup, 0)
    ref = 0.5 * (grey0 + grey1)
    print(json.dumps({"setup": setup, "format": "GRAY8", "frames_per_s": round(ref), "first": round(grey0), "last": round(grey1),
                      "noise_pct": round(100 * abs(grey0 - grey1) / ref, 2)}), flush=True)
    for fmt, (r, rates) in res.items():
        print(json.dumps({"setup": setup, "format": NAMES[fmt], "frames_per_s": round(r), "vs_gray8": round(r / ref, 4),
                          "windows": [round(x) for x in rates]}), flush=True)
