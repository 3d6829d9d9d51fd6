#!/usr/bin/env python3
"""What handing a retiring keyframe's depths on to its successor costs, and what it does to the alignment on the bench stream
(DESIGN.md 5m). One JSON line per measurement on stdout.

  kernels   device time per launch of k_kf_handover_claim and k_kf_handover_apply next to k_kf_fuse_depth in the same process
            (rebvio_hip_profile_*: HIP events around every launch), alternating, three rounds, and the wall time of the synchronous
            calls, on the two maps of tools/kf_align_rate.py: a map of the 640x480 bench stream seven pairs behind its keyframe, at
            the alignment's pose, into that map's own snapshot, and a detected 65 536-keyline map against a 65 536-keyline snapshot
  effect    tools/kf_fuse_rate.py's `effect` stream (640x480 bench stream, a keyframe every 10 records, fusion on): `used` and cost of
            rebvio_hip_map_keyframe_align per pair behind every mark with and without the hand-over at the mark, both warm-started
            alike, and the number of keylines of each retired keyframe that pass the default cloud filter
  host      rebvio::Rebvio (rebvio_replay) on the bench stream with --kf-align --kf-fuse, with and without --kf-handover (a keyframe
            every 10 records), processes alternating, `--rounds` times each

    tools/kf_handover_rate.py [kernels] [effect] [host] [--frames N] [--rounds R] [--reps K]"""
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
COUNTS = ("candidates", "associated", "out_of_range", "claimed", "adopted", "kept", "conflicts")
KERNELS = ("k_kf_fuse_depth", "k_kf_handover_claim", "k_kf_handover_apply")


def wall(call, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    return round((time.perf_counter() - t0) / reps * 1e6, 1)


def counts(h):
    return {k: getattr(h, k) for k in COUNTS}


def time_handover(B, ctx, src, dst, m, reps, what, R, t):
    """src: the outgoing snapshot with normals (the yardstick fuses m into it `reps` times over); dst: the successor (after the first
    call its adopted slots are kept ones: the kernels' loads, gathers and claims per launch are a first call's, its stores are not)"""
    out = dict(what=what, keylines=m.size(), kf_size=len(src.download()[0]), dst_size=len(dst.download()[0]), reps=reps)
    out["first"] = counts(dst.handover_depth(src, m, R, t))      # warm: scratch allocated
    src.fuse_depth(m, R, t)
    for round_ in range(3):                                      # alternating, three rounds: the table's own spread
        for names, call in ((KERNELS[:1], lambda: src.fuse_depth(m, R, t)), (KERNELS[1:], lambda: dst.handover_depth(src, m, R, t))):
            ctx.profile(True, only="k_kf_*")
            ctx.profile_reset()
            for _ in range(reps):
                call()
            prof = ctx.profile_read()
            for name in names:
                out.setdefault(name + "_us", []).append(round(prof[name][0], 2))
            ctx.profile(False)
    out["handover_call_wall_us"] = wall(lambda: dst.handover_depth(src, m, R, t), reps)
    out["fuse_call_wall_us"] = wall(lambda: src.fuse_depth(m, R, t), reps)
    out["last"] = counts(dst.handover_depth(src, m, R, t))
    for name in KERNELS:
        v = out[name + "_us"]
        out[name + "_median_us"], out[name + "_spread_us"] = float(np.median(v)), round(max(v) - min(v), 2)
    src.release()
    dst.release()
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
    time_handover(B, ctx, snap, maps[9].keyframe_snapshot(), maps[9], args.reps,
                  f"640x480 bench stream, map 7 pairs behind its keyframe, at the alignment's pose (status {A.status}, used {A.used})",
                  np.array(A.R), np.array(A.t))
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
    time_handover(B, ctx, snap, m.keyframe_snapshot(), m, args.reps,
                  f"{W}x{H}, keylines_max 65536, a detected map against a 65 536-keyline snapshot, R = I, t = (0.01, 0, 0)", np.eye(3),
                  np.array([0.01, 0.0, 0.0]))
    ctx.close()


def passing(snap):
    """keylines of a snapshot under the default cloud filter, and their mean sigma_rho / rho"""
    prs, mt = snap.download()
    ok = (mt >= 2) & (prs[:, 3] <= 0.5 * prs[:, 2]) & (prs[:, 2] >= 1e-3) & (prs[:, 2] <= 20)
    return int(ok.sum()), round(float((prs[:, 3] / prs[:, 2])[ok].mean()), 4) if ok.any() else None


def effect(args):
    import torch  # noqa: F401
    from rebvio_amd import backend as B
    n = 41
    ctx, maps = bench_maps(B, n)
    snaps = {"plain": None, "handover": None}
    guess = {"plain": None, "handover": None}
    keyframe = 0
    for k in range(n - 1):
        out = ctx.track_pair(maps[k], maps[k + 1])
        new = maps[k + 1]
        if k % 10 == 9:                                        # the mark, as rebvio::Rebvio places it: behind the pair, on its new map
            new.mark_keyframe()
            keyframe += 1
            row = dict(what="mark", pair=k, keyframe=keyframe, keylines=new.size())
            for name in snaps:
                old, g = snaps[name], guess[name]
                s = new.keyframe_snapshot()
                s.add_normals(new)
                if old:
                    row[name + "_retired_pass_filter"], row[name + "_retired_mean_rel_sigma"] = passing(old)
                    if name == "handover" and g:
                        p = new.keyframe_align(old, None, *g)
                        row["outgoing_status"], row["outgoing_used"] = p.status, p.used
                        if p.status == 0:
                            row["handover"] = counts(s.handover_depth(old, new, np.array(p.R), np.array(p.t)))
                    old.release()
                row[name + "_new_pass_filter"], row[name + "_new_mean_rel_sigma"] = passing(s)
                snaps[name], guess[name] = s, None
            print(json.dumps(row), flush=True)
            continue
        if not snaps["plain"]:
            continue
        row = dict(what="effect", pair=k, keyframe=keyframe, behind_mark=k % 10 + 1, keylines=new.size(), track_status=out.status)
        for name, s in snaps.items():
            g = guess[name]
            p = new.keyframe_align(s, None, *(g if g else (None, None)))
            row.update({name + "_status": p.status, name + "_used": p.used, name + "_cost": round(p.cost, 1),
                        name + "_cost_per_term": round(p.cost / max(p.used, 1), 4)})
            if p.status == 0:
                guess[name] = (np.array(p.R), np.array(p.t))
                f = s.fuse_depth(new, *guess[name])            # fusion on in both
                row[name + "_fused"] = f.fused
        print(json.dumps(row), flush=True)
    for name, s in snaps.items():
        if s:
            print(json.dumps(dict(what="last keyframe", name=name, pass_filter=passing(s)[0], mean_rel_sigma=passing(s)[1])), flush=True)
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
            str(cam.cx), str(cam.cy), "--keylines", "15000", "16000", "--out", os.path.join(d, "o.txt"), "--kf-align", os.path.join(d, "a.txt"),
            "--kf-fuse", os.path.join(d, "f.txt")]
    rates = {"fuse": [], "handover": []}
    ho = os.path.join(d, "h.txt")
    for _ in range(args.rounds):
        for kind in rates:
            r = subprocess.run(base + (["--kf-handover", ho] if kind == "handover" else []), capture_output=True, text=True, timeout=600)
            m = re.search(r"= (\d+) frames/s", r.stderr)
            if r.returncode != 0 or not m:
                print(json.dumps(dict(what="host class", kind=kind, rc=r.returncode, stderr=r.stderr[-400:])), flush=True)
                return
            rates[kind].append(int(m.group(1)))
    med = {k: float(np.median(v)) for k, v in rates.items()}
    hz = np.array([[int(x) for x in line.split()[2:]] for line in open(ho)])
    print(json.dumps(dict(what="rebvio::Rebvio on the 640x480 bench stream (rebvio_replay), frames/s first to last record", frames=n,
                          with_kf_fuse=rates["fuse"], with_kf_handover=rates["handover"], median_fuse=med["fuse"],
                          median_handover=med["handover"], ratio=round(med["handover"] / med["fuse"], 4), handover_records=len(hz),
                          adopted_mean=round(float(hz[:, 4].mean()), 1) if len(hz) else None,
                          associated_mean=round(float(hz[:, 1].mean()), 1) if len(hz) else None)), flush=True)


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
