#!/usr/bin/env python3
"""What the depth fusion into a keyframe snapshot costs, and what it does to the alignment on the bench stream.
One JSON line per measurement on stdout.

  kernels   device time per launch of k_kf_fuse_depth next to k_kf_align_sums in the same process (rebvio_hip_profile_*: HIP events
            around every launch) and the wall time of a synchronous rebvio_hip_kf_snapshot_fuse_depth call, on the two maps of
            tools/kf_align_rate.py: a map of the 640x480 bench stream seven pairs behind its keyframe, fused at the alignment's pose,
            and a detected 65 536-keyline map against a 65 536-keyline snapshot
  effect    the 640x480 bench stream, a keyframe every 10 records: `used` of rebvio_hip_map_keyframe_align per pair behind the mark
            against a snapshot that is fused with every aligned map and against one that is not, both warm-started alike
  host      rebvio::Rebvio (rebvio_replay) on the bench stream with --kf-align and with --kf-fuse (a keyframe every 10 records),
            processes alternating, `--rounds` times each

    tools/kf_fuse_rate.py [kernels] [effect] [host] [--frames N] [--rounds R] [--reps K]"""
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
COUNTS = ("candidates", "associated", "fused", "gated", "flat", "clamped")


def wall(call, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    return round((time.perf_counter() - t0) / reps * 1e6, 1)


def counts(f):
    return {k: getattr(f, k) for k in COUNTS}


def time_fuse(B, ctx, snap, m, reps, what, R, t):
    """snap: a snapshot with normals (it is fused `reps` times over: the kernel's work per launch is what a first fusion's is up to the
    keylines whose update the earlier ones gated); m: the current map"""
    out = dict(what=what, keylines=m.size(), kf_size=len(snap.download()[0]), reps=reps)
    oa = B.default_kf_align_opts(ctx, max_iter=0)
    out["first"] = counts(snap.fuse_depth(m, R, t))            # warm: scratch allocated
    m.keyframe_align(snap, oa, R, t)
    for round_ in range(3):                                    # the two kernels alternating, three rounds: the table's own spread
        for name, call in (("k_kf_align_sums", lambda: m.keyframe_align(snap, oa, R, t)), ("k_kf_fuse_depth", lambda: snap.fuse_depth(m, R, t))):
            ctx.profile(True, only="k_kf_*")
            ctx.profile_reset()
            for _ in range(reps):
                call()
            out.setdefault(name + "_us", []).append(round(ctx.profile_read()[name][0], 2))
            ctx.profile(False)
    out["fuse_call_wall_us"] = wall(lambda: snap.fuse_depth(m, R, t), reps)
    out["align_call_iter0_wall_us"] = wall(lambda: m.keyframe_align(snap, oa, R, t), reps)
    out["last"] = counts(snap.fuse_depth(m, R, t))
    snap.release()
    print(json.dumps(out), flush=True)


def bench_maps(B, n):
    from rebvio_amd import synth
    frames, cam = synth.render_stream(640, 480, 24)
    ctx = B.Context(B.default_params(480, 640, fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=15000, keylines_max=16000))
    idx = synth.pingpong_indices(24, n)
    return ctx, [ctx.detect_u8(frames[i], k * 50000) for k, i in enumerate(idx)]


def kernels(args):
    import torch  # noqa: F401
    from rebvio_amd import backend as B
    from rebvio_amd import synth
    ctx, maps = bench_maps(B, 10)
    for k in range(2):
        ctx.track_pair(maps[k], maps[k + 1])
    maps[2].mark_keyframe()
    snap = maps[2].keyframe_snapshot()  # at the mark, before the map serves as an old map
    snap.add_normals(maps[2])
    for k in range(2, 9):
        ctx.track_pair(maps[k], maps[k + 1])
    P = maps[9].keyframe_pose(snap)
    A = maps[9].keyframe_align(snap, None, np.array(P.R), np.array(P.t))
    time_fuse(B, ctx, snap, maps[9], args.reps, f"640x480 bench stream, map 7 pairs behind its keyframe, at the alignment's pose (status {A.status}, "
              f"used {A.used})", np.array(A.R), np.array(A.t))
    ctx.close()
    small, qcam = synth.render_stream(576, 475, 3)
    big = np.ascontiguousarray(np.kron(small, np.ones((1, 4, 4), np.uint8)))
    H, W = big.shape[1:]
    ctx = B.Context(B.default_params(H, W, fm=qcam.fm * 4, cx=qcam.cx * 4 + 1.5, cy=qcam.cy * 4 + 1.5, keylines_ref=60000, keylines_max=65536))
    mk, m = (ctx.detect_u8(big[i], i * 50000) for i in range(2))
    kf = mk.keylines()
    rng = np.random.default_rng(1)
    kf["matches"] = 3
    kf["rho"] = rng.uniform(0.2, 2.0, len(kf)).astype(np.float32)
    kf["sigma_rho"] = (0.05 * kf["rho"]).astype(np.float32)
    mk.upload(kf)
    snap = mk.keyframe_snapshot()
    snap.add_normals(mk)
    time_fuse(B, ctx, snap, m, args.reps, f"{W}x{H}, keylines_max 65536, a detected map against a 65 536-keyline snapshot, R = I, t = (0.01, 0, 0)",
              np.eye(3), np.array([0.01, 0.0, 0.0]))
    ctx.close()


def effect(args):
    import torch  # noqa: F401
    from rebvio_amd import backend as B
    n = 41
    ctx, maps = bench_maps(B, n)
    plain = fused = None
    guess = {}
    for k in range(n - 1):
        out = ctx.track_pair(maps[k], maps[k + 1])
        new = maps[k + 1]
        if k % 10 == 9:                                        # the mark, as rebvio::Rebvio places it: behind the pair, on its new map
            new.mark_keyframe()
            for s in (plain, fused):
                if s:
                    s.release()
            plain, fused = new.keyframe_snapshot(), new.keyframe_snapshot()
            plain.add_normals(new)
            fused.add_normals(new)
            guess = {"plain": None, "fused": None}
            continue
        if not plain:
            continue
        row = dict(what="effect", pair=k, behind_mark=k % 10 + 1 if k % 10 != 9 else 0, keylines=new.size(), track_status=out.status)
        for name, s in (("plain", plain), ("fused", fused)):
            g = guess[name]
            p = new.keyframe_align(s, None, *(g if g else (None, None)))
            row.update({name + "_status": p.status, name + "_used": p.used, name + "_cost": round(p.cost, 1)})
            if p.status == 0:
                guess[name] = (np.array(p.R), np.array(p.t))
                if name == "fused":
                    row["fusion"] = counts(s.fuse_depth(new, *guess[name]))
                    prs, mt = s.download()
                    ok = mt >= 2
                    row["kf_pass_filter"] = int((ok & (prs[:, 3] <= 0.5 * prs[:, 2]) & (prs[:, 2] >= 1e-3) & (prs[:, 2] <= 20)).sum())
                    row["kf_mean_rel_sigma"] = round(float((prs[:, 3] / prs[:, 2])[ok & (prs[:, 2] > 0)].mean()), 4)
        print(json.dumps(row), flush=True)
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
    rates = {"align": [], "fuse": []}
    lines = {}
    for _ in range(args.rounds):
        for kind in ("align", "fuse"):
            path = os.path.join(d, kind + ".txt")
            r = subprocess.run(base + ["--kf-" + kind, path], capture_output=True, text=True, timeout=300)
            m = re.search(r"= (\d+) frames/s", r.stderr)
            if r.returncode != 0 or not m:
                print(json.dumps(dict(what="host class", kind=kind, rc=r.returncode, stderr=r.stderr[-400:])), flush=True)
                return
            rates[kind].append(int(m.group(1)))
            lines[kind] = [line.split() for line in open(path)]
    med = {k: float(np.median(v)) for k, v in rates.items()}
    fz = np.array([[int(x) for x in f[1:]] for f in lines["fuse"]])
    print(json.dumps(dict(what="rebvio::Rebvio on the 640x480 bench stream (rebvio_replay), frames/s first to last record", frames=n,
                          with_kf_align=rates["align"], with_kf_fuse=rates["fuse"], median_align=med["align"], median_fuse=med["fuse"],
                          ratio=round(med["fuse"] / med["align"], 4), pose_records=len(lines["align"]), fuse_records=len(lines["fuse"]),
                          fused_mean=round(float(fz[:, 2].mean()), 1) if len(fz) else None,
                          associated_mean=round(float(fz[:, 1].mean()), 1) if len(fz) else None)), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernels", "effect", "host"])
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    if "kernels" in a.what:
        kernels(a)
    if "effect" in a.what:
        effect(a)
    if "host" in a.what:
        host(a)
