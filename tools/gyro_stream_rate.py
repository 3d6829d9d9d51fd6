#!/usr/bin/env python3
"""Frames/s of the streaming driver on the bench stream (640x480, 8 frames ping-pong, device-resident GRAY8 frames) without and
with per-frame gyro rotations, in one process:
    u8        rebvio_hip_push_frame_u8_device                (what bench.py times)
    gyro-null rebvio_hip_push_frame_px_gyro_device, R_gyro = NULL
    gyro      rebvio_hip_push_frame_px_gyro_device, every frame with the scene's rotation over its interval plus a small error
  gyro_stream_rate.py [steps] [warmup] [--repeat N] [--no-bind]
The three take turns, --repeat windows each, so that a drift of the machine reaches all of them; one JSON line per entry with the
median rate, its windows, and the kernel launches per frame (profiler call counts over a short run of its own, not timed)."""
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

ap = argparse.ArgumentParser()
ap.add_argument("steps", nargs="?", type=int, default=2000)
ap.add_argument("warmup", nargs="?", type=int, default=500)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--no-bind", action="store_true")
a = ap.parse_args()

if not a.no_bind:  # like bench.py: the CPUs of the GPU's NUMA node
    _pr = torch.cuda.get_device_properties(0)
    shard.bind_to_gpu_numa_node(f"{_pr.pci_domain_id:04x}:{_pr.pci_bus_id:02x}:{_pr.pci_device_id:02x}.0")

W, H, NF = 640, 480, 8
frames, cam = synth.render_stream(W, H, NF)
params = B.default_params(H, W, fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=15000, keylines_max=16000)
NPX = W * H
PROFILED = 96
total = a.warmup + a.repeat * a.steps + PROFILED + 8
order = synth.pingpong_indices(NF, total)


def rodrigues(w):
    th = np.sqrt((w * w).sum())
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    return np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / (th * th)) * (K @ K)


def rotations():
    """[k]: frame order[k-1] -> order[k], the scene's own rotation times a gyro error of up to 0.004 rad per axis"""
    scene = synth.make_scene(0, 1.0)
    rng = np.random.Generator(np.random.PCG64(5))
    poses = [synth.pose(scene, i)[0] for i in range(NF)]
    out = [np.eye(3, dtype=np.float32)]
    for i, j in zip(order[:-1], order[1:]):
        out.append(np.ascontiguousarray(((poses[i].T @ poses[j]).T @ rodrigues(rng.uniform(-0.004, 0.004, 3))).astype(np.float32)))
    return out


ROT = rotations()


class Entry:
    def __init__(self, name):
        self.name = name
        self.ctx = B.Context(params)
        self.dev = self.ctx.upload_frames(frames)
        self.k = 0
        self.rates = []
        self.matches = []

    def push(self):
        k, ctx = self.k, self.ctx
        addr = self.dev + int(order[k]) * NPX
        if self.name == "u8":
            out, _ = ctx.push_frame_u8_device(addr, k * 50000)
        else:
            out, _ = ctx.push_frame_px_gyro_device(addr, B.PX_GRAY8, ROT[k] if self.name == "gyro" else None, None, k * 50000)
        if out.status >= 0:
            self.matches.append(out.klm_num if out.status == 0 else -1)
        self.k += 1

    def window(self, n, timed=True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            self.push()
        torch.cuda.synchronize()
        if timed:
            self.rates.append(n / (time.perf_counter() - t0))


entries = [Entry(n) for n in ("u8", "gyro-null", "gyro")]
for e in entries:
    e.window(a.warmup, timed=False)
for _ in range(a.repeat):
    for e in entries:
        e.window(a.steps)
for e in entries:
    e.ctx.profile_reset()
    e.ctx.profile(True)
    e.window(PROFILED, timed=False)
    calls = {name: c for name, (_, c) in e.ctx.profile_read().items()}
    e.ctx.profile(False)
    e.ctx.flush()
    good = [m for m in e.matches if m >= 0]
    print(json.dumps({"entry": e.name, "frames_per_s": round(statistics.median(e.rates)), "windows": [round(r) for r in e.rates],
                      "launches_per_frame": round(sum(calls.values()) / PROFILED, 3), "pairs_reported": len(e.matches),
                      "pairs_tracked": len(good), "mean_klm_num": round(float(np.mean(good))) if good else 0}), flush=True)
    e.ctx.close()
