#!/usr/bin/env python3
"""What the keyframe snapshot and the keyframe-to-current pose cost.  One JSON line per measurement on stdout.

  kernels   device time per launch of k_kf_snapshot, k_kf_pose_sums and k_kf_pose_step (rebvio_hip_profile_*: HIP events around every
            launch) and the wall time of a synchronous rebvio_hip_map_keyframe_pose call at max_iter 0 and 8, on a map of the
            640x480 bench stream seven pairs behind its keyframe (~15 k keylines) and on a 65 536-keyline map whose every keyline
            continues a keyline of the keyframe
  host      rebvio::Rebvio (rebvio_replay) on the bench stream without and with a registered keyframe-pose callback (--kf-pose, a
            keyframe every 10 records), processes alternating, `--rounds` times each; the callback's price as the ratio of the medians

    tools/kf_pose_rate.py [kernels] [host] [--frames N] [--rounds R] [--reps K]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_pose(B, ctx, snap, mk, m, reps, what):
    """snap: the keyframe's snapshot; mk: the keyframe map (snapshotted again for the kernel's own time); m: the current map"""
    n_kf = len(snap.download()[0])
    out = dict(what=what, keylines=m.size(), kf_size=n_kf, reps=reps)
    for it in (0, 8):
        opts = B.default_kf_pose_opts(max_iter=it)
        p = m.keyframe_pose(snap, opts)  # warm: scratch allocated
        ctx.profile(True, only="k_kf_*")
        ctx.profile_reset()
        t0 = time.perf_counter()
        for _ in range(reps):
            m.keyframe_pose(snap, opts)
        wall_prof = (time.perf_counter() - t0) / reps * 1e6
        prof = ctx.profile_read()
        ctx.profile(False)
        t0 = time.perf_counter()
        for _ in range(reps):
            m.keyframe_pose(snap, opts)
        wall = (time.perf_counter() - t0) / reps * 1e6
        out.update({f"iter{it}_sync_call_wall_us": round(wall, 1), f"iter{it}_sync_call_wall_us_profiler_on": round(wall_prof, 1),
                    f"iter{it}_status": p.status, f"iter{it}_candidates": p.candidates, f"iter{it}_used": p.used})
        if it == 8:
            out.update({k + "_us": round(prof[k][0], 2) for k in ("k_kf_claim", "k_kf_count", "k_kf_emit", "k_kf_pose_sums", "k_kf_pose_step")})
    ctx.profile(True, only="k_kf_snapshot")
    ctx.profile_reset()
    extra = [mk.keyframe_snapshot() for _ in range(min(reps, 32))]
    mk.keylines()  # (waits for the track stream)
    out["k_kf_snapshot_us"] = round(ctx.profile_read()["k_kf_snapshot"][0], 2)
    ctx.profile(False)
    for s in extra + [snap]:
        s.release()
    print(json.dumps(out), flush=True)


def kernels(args):
    import torch  # noqa: F401
    from rebvio_amd import backend as B
    from rebvio_amd import synth
    frames, cam = synth.render_stream(640, 480, 10)
    ctx = B.Context(B.default_params(480, 640, fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=15000, keylines_max=16000))
    maps = [ctx.detect_u8(frames[i], i * 50000) for i in range(10)]
    for k in range(2):
        ctx.track_pair(maps[k], maps[k + 1])
    maps[2].mark_keyframe()
    snap = maps[2].keyframe_snapshot()  # at the mark, before the map serves as an old map
    for k in range(2, 9):
        ctx.track_pair(maps[k], maps[k + 1])
    time_pose(B, ctx, snap, maps[2], maps[9], args.reps, "640x480 bench stream, map 7 pairs behind its keyframe")
    ctx.close()
    small, qcam = synth.render_stream(576, 475, 2)
    big = np.ascontiguousarray(np.kron(small, np.ones((1, 4, 4), np.uint8)))
    H, W = big.shape[1:]
    ctx = B.Context(B.default_params(H, W, fm=qcam.fm * 4, cx=qcam.cx * 4 + 1.5, cy=qcam.cy * 4 + 1.5, keylines_ref=60000, keylines_max=65536))
    mk, m = (ctx.detect_u8(big[i], i * 50000) for i in range(2))
    kf, kl = mk.keylines(), m.keylines()
    rng = np.random.default_rng(1)
    kf["matches"] = 3
    kf["rho"] = rng.uniform(0.2, 2.0, len(kf)).astype(np.float32)
    kf["sigma_rho"] = (0.05 * kf["rho"]).astype(np.float32)
    mk.upload(kf)
    n = min(len(kf), len(kl))
    kl["match_id_keyframe"] = -1
    kl["match_id_keyframe"][:n] = np.arange(n)
    kl["pos_img"][:n] = kf["pos_img"][:n] + rng.normal(0, 0.5, (n, 2)).astype(np.float32)
    m.upload(kl)
    time_pose(B, ctx, mk.keyframe_snapshot(), mk, m, args.reps, f"{W}x{H}, keylines_max 65536, every keyline a correspondence")
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
    rates = {"plain": [], "pose": []}
    poses = 0
    for _ in range(args.rounds):
        for kind in ("plain", "pose"):
            r = subprocess.run(base + (["--kf-pose", os.path.join(d, "p.txt")] if kind == "pose" else []), capture_output=True, text=True, timeout=300)
            m = re.search(r"= (\d+) frames/s", r.stderr)
            if r.returncode != 0 or not m:
                print(json.dumps(dict(what="host class", kind=kind, rc=r.returncode, stderr=r.stderr[-400:])), flush=True)
                return
            rates[kind].append(int(m.group(1)))
            mp = re.search(r"kf_poses=(\d+)", r.stderr)
            if mp:
                poses = int(mp.group(1))
    med = {k: float(np.median(v)) for k, v in rates.items()}
    status = [int(line.split()[1]) for line in open(os.path.join(d, "p.txt"))]
    print(json.dumps(dict(what="rebvio::Rebvio on the 640x480 bench stream (rebvio_replay), frames/s first to last record", frames=n,
                          plain=rates["plain"], with_kf_pose_callback=rates["pose"], median_plain=med["plain"], median_pose=med["pose"],
                          ratio=round(med["pose"] / med["plain"], 4), poses=poses, status0=status.count(0), status3=status.count(3),
                          status2=status.count(2))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernels", "host"])
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    if "kernels" in a.what:
        kernels(a)
    if "host" in a.what:
        host(a)
