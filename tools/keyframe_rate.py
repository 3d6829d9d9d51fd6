#!/usr/bin/env python3
"""What the keyframe entries cost.  One JSON line per measurement on stdout.

Device time of k_mark_keyframe and of k_kf_claim / k_kf_count / k_kf_emit (rebvio_hip_profile_*: HIP events around every launch)
and the wall time of a synchronous rebvio_hip_map_keyframe_matches call and of a queued rebvio_hip_map_mark_keyframe call, on a
map of the 640x480 bench stream seven pairs behind its keyframe (~15 k keylines) and on a 65 536-keyline map whose keyframe ids are
random (every keyline a claimant, about 63 % of the slots claimed).

    tools/keyframe_rate.py [--reps K]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_map(ctx, m, kf_size, reps, what):
    n = m.size()
    rec, count = m.keyframe_matches(kf_size, return_count=True)  # warm: scratch allocated
    ctx.profile(True, only="k_kf_*")
    ctx.profile_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        m.keyframe_matches(kf_size)
    wall = (time.perf_counter() - t0) / reps * 1e6
    prof = ctx.profile_read()
    ctx.profile(True, only="k_mark_keyframe")
    ctx.profile_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        m.mark_keyframe()
    mark_wall = (time.perf_counter() - t0) / reps * 1e6
    m.keylines()  # (waits for the track stream)
    mark = ctx.profile_read()["k_mark_keyframe"][0]
    ctx.profile(False)
    print(json.dumps(dict(what=what, keylines=n, kf_size=kf_size, records=count, claimants=int(rec["claimants"].sum()), reps=reps,
                          k_kf_claim_us=round(prof["k_kf_claim"][0], 2), k_kf_count_us=round(prof["k_kf_count"][0], 2),
                          k_kf_emit_us=round(prof["k_kf_emit"][0], 2), sync_call_wall_us=round(wall, 1),
                          k_mark_keyframe_us=round(mark, 2), mark_call_wall_us_profiler_on=round(mark_wall, 1))), flush=True)


def main(args):
    import torch  # noqa: F401
    from rebvio_amd import backend as B
    from rebvio_amd import synth
    frames, cam = synth.render_stream(640, 480, 8)
    ctx = B.Context(B.default_params(480, 640, fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=15000, keylines_max=16000))
    maps = [ctx.detect_u8(frames[i], i * 50000) for i in range(8)]
    n0 = maps[0].size()
    maps[0].mark_keyframe()
    kf = [ctx.track_pair(maps[k], maps[k + 1]).kf_matches for k in range(7)]
    time_map(ctx, maps[-1], n0, args.reps, f"640x480 bench stream, map 7 pairs behind its keyframe (kf_matches per pair {kf})")
    ctx.close()
    small, qcam = synth.render_stream(576, 475, 2)
    big = np.ascontiguousarray(np.kron(small, np.ones((1, 4, 4), np.uint8)))
    H, W = big.shape[1:]
    ctx = B.Context(B.default_params(H, W, fm=qcam.fm * 4, cx=qcam.cx * 4 + 1.5, cy=qcam.cy * 4 + 1.5, keylines_ref=60000, keylines_max=65536))
    m = max((ctx.detect_u8(big[i], i * 50000) for i in range(2)), key=lambda x: x.size())
    kl = m.keylines()
    rng = np.random.default_rng(1)
    kl["match_id_keyframe"] = rng.integers(0, len(kl), len(kl))
    kl["sigma_rho"] = rng.uniform(0.0, 1.0, len(kl)).astype(np.float32)
    m.upload(kl)
    time_map(ctx, m, len(kl), args.reps, f"{W}x{H}, keylines_max 65536, random keyframe ids")
    ctx.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    main(ap.parse_args())
