#!/usr/bin/env python3
"""Frames/s and mean keylines of the streaming driver with detection masks, 640x480, one stream and 8 lanes of a batch
(device-resident frames), for four cases:
  none        no mask (the unmasked candidate kernel)
  ones        an all-ones static mask (rebvio_hip_set_detection_mask): the masked kernel, the keylines of `none`
  bottom3     a static mask that excludes the bottom third of the frame
  per-frame   the bottom-third mask as a per-frame device mask (*_masked_device entries), a different buffer every frame
  mask_rate.py [steps] [warmup] [--cases none,ones,bottom3,per-frame] [--setups stream,batch8] [--repeat N]
Prints one JSON line per (setup, case) with the rate, its ratio to `none` in the same setup (median of --repeat windows; `none`
is measured first and again last: the spread of the two is the run-to-run noise of the setup) and the mean keyline count of the
pairs' new maps."""
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

CASES = ["none", "ones", "bottom3", "per-frame"]

ap = argparse.ArgumentParser()
ap.add_argument("steps", nargs="?", type=int, default=2000)
ap.add_argument("warmup", nargs="?", type=int, default=500)
ap.add_argument("--cases", default=",".join(CASES))
ap.add_argument("--setups", default="stream,batch8")
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--no-bind", action="store_true")
a = ap.parse_args()

if not a.no_bind:  # like bench.py: the CPUs of the GPU's NUMA node
    _pr = torch.cuda.get_device_properties(0)
    shard.bind_to_gpu_numa_node(f"{_pr.pci_domain_id:04x}:{_pr.pci_bus_id:02x}:{_pr.pci_device_id:02x}.0")

W, H, NF = 640, 480, 24
cam = synth.Camera.for_size(W, H)
params = B.default_params(H, W, fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=15000, keylines_max=16000)
ONES = np.ones((H, W), np.uint8)
BOTTOM3 = np.ones((H, W), np.uint8)
BOTTOM3[H - H // 3:] = 0
NMASK = 8  # per-frame masks: a ring of device buffers holding the same mask

_grey = {}


def grey_stream(stream_id):
    if stream_id not in _grey:
        _grey[stream_id] = synth.render_stream(W, H, NF, stream_id=stream_id)[0]
    return _grey[stream_id]


def window(push, k0, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(k0, k0 + n):
        push(k)
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def measure(setup, case):
    order = synth.pingpong_indices(NF, a.warmup + a.repeat * a.steps + 8)
    kl = []
    L = 8 if setup == "batch8" else 1
    if setup == "batch8":
        obj = B.Batch(params, L)
        ctxs = obj.lanes
    else:
        obj = B.Context(params)
        ctxs = [obj]
    devs = [c.upload_frames(grey_stream(l)) for l, c in enumerate(ctxs)]
    if case in ("ones", "bottom3"):
        for c in ctxs:
            c.set_detection_mask(ONES if case == "ones" else BOTTOM3)
    mdevs = [c.upload_frames(np.stack([BOTTOM3] * NMASK)) for c in ctxs] if case == "per-frame" else None

    def take(n):
        if n >= 0:
            kl.append(n)

    def push(k):
        fr = [d + int(order[k]) * W * H for d in devs]
        ms = [m + (k % NMASK) * W * H for m in mdevs] if mdevs else None
        if setup == "batch8":
            _, ns = obj.push_px_masked_device(fr, B.PX_GRAY8, ms, k * 50000) if ms else obj.push_u8_device(fr, k * 50000)
            for l in range(L):
                take(ns[l])
        else:
            _, n = obj.push_frame_px_masked_device(fr[0], B.PX_GRAY8, ms[0], k * 50000) if ms else obj.push_frame_u8_device(fr[0], k * 50000)
            take(n)

    window(push, 0, a.warmup)
    kl.clear()
    rates = [window(push, a.warmup + r * a.steps, a.steps) for r in range(a.repeat)]
    obj.flush()
    obj.close()
    return statistics.median(rates) * L, rates, float(np.mean(kl)) if kl else float("nan")


cases = a.cases.split(",")
for setup in a.setups.split(","):
    none0, _, kl_none = measure(setup, "none")
    res = {c: measure(setup, c) for c in cases if c != "none"}
    none1, _, _ = measure(setup, "none")
    ref = 0.5 * (none0 + none1)
    print(json.dumps({"setup": setup, "case": "none", "frames_per_s": round(ref), "first": round(none0), "last": round(none1),
                      "noise_pct": round(100 * abs(none0 - none1) / ref, 2), "mean_keylines": round(kl_none, 1)}), flush=True)
    for c, (r, rates, k) in res.items():
        print(json.dumps({"setup": setup, "case": c, "frames_per_s": round(r), "vs_none": round(r / ref, 4),
                          "windows": [round(x) for x in rates], "mean_keylines": round(k, 1)}), flush=True)
