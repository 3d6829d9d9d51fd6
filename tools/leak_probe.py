"""Create / use / destroy many contexts in one process and report what stays allocated: the library's own count of the device
buffers, pinned buffers, events and streams it holds (rebvio_hip_test_live_resources, exact) and the device memory in use
(device-wide, so other processes on the GPU show in it: reported, not judged). Exit status 1 if the count has not returned to
its starting value.
    python tools/leak_probe.py [--rounds 100]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=100)
    a = ap.parse_args()
    import torch
    from rebvio_amd import backend as B
    from rebvio_amd import synth
    B.lib()
    frames, cam = synth.render_stream(640, 480, 4)
    kw = dict(fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=15000, keylines_max=16000)
    live0 = B.test_live_resources()
    used, live = [], []
    for r in range(a.rounds):
        ctx = B.Context(B.default_params(480, 640, **kw))
        dev = ctx.upload_frames(frames)
        for k in range(8):
            ctx.push_frame_u8_device(dev + (k % 4) * 640 * 480, k * 50000)
        ctx.flush()
        ctx.close()
        del ctx
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        used.append((total - free) / 2**20)
        live.append(B.test_live_resources())
        if r % 10 == 0:
            print(f"round {r}: {live[-1] - live0} resources held, {used[-1]:.1f} MiB in use", flush=True)
    print(f"first {used[0]:.1f} MiB, after 10 {used[min(10, len(used) - 1)]:.1f} MiB, last {used[-1]:.1f} MiB")
    print(f"resources held: {live0} at the start, {live[-1]} at the end, at most {max(live)} after a round")
    return 0 if all(v == live0 for v in live) else 1


if __name__ == "__main__":
    sys.exit(main())
