#!/usr/bin/env python3
"""What the snapshot normals and the alignment through the distance field cost, and from how far it converges.
One JSON line per measurement on stdout.

  kernels   device time per launch of k_kf_snapshot_normals, k_kf_align_sums and k_kf_pose_step (rebvio_hip_profile_*: HIP events
            around every launch) and the wall time of a synchronous rebvio_hip_map_keyframe_align call at max_iter 0 and 8, next to
            rebvio_hip_map_keyframe_pose on the same map in the same process: on a map of the 640x480 bench stream seven pairs behind
            its keyframe (~15 k keylines; the alignment starts from the chain's pose) and on a detected 65 536-keyline map against a
            65 536-keyline snapshot (the pose entry there: every keyline a correspondence, as tools/kf_pose_rate.py sets it up)
  host      rebvio::Rebvio (rebvio_replay) on the bench stream with --kf-pose and with --kf-align (a keyframe every 10 records),
            processes alternating, `--rounds` times each
  basin     the 160x120 scene of the tests (keyframe keylines crafted behind a known motion against a detected map): the error of
            the restatement (tests/kf_align_ref.py) and of the device from the true motion, started 0.002 .. 0.05 rad (and four
            times that in translation units) off it, with and without normals

    tools/kf_align_rate.py [kernels] [host] [basin] [--frames N] [--rounds R] [--reps K]"""
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


def wall(call, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    return round((time.perf_counter() - t0) / reps * 1e6, 1)


def time_align(B, ctx, snap, mk, m, reps, what, guess=None):
    """snap: the keyframe's snapshot with normals; mk: a map to take normals from for the kernel's own time; m: the current map"""
    n_kf = len(snap.download()[0])
    out = dict(what=what, keylines=m.size(), kf_size=n_kf, reps=reps)
    R0, t0 = guess if guess is not None else (None, None)
    for it in (0, 8):
        oa, op = B.default_kf_align_opts(ctx, max_iter=it), B.default_kf_pose_opts(max_iter=it)
        a = m.keyframe_align(snap, oa, R0, t0)  # warm: scratch allocated
        p = m.keyframe_pose(snap, op)
        ctx.profile(True, only="k_kf_*")
        ctx.profile_reset()
        wall_prof = wall(lambda: m.keyframe_align(snap, oa, R0, t0), reps)
        prof = ctx.profile_read()
        ctx.profile(False)
        out.update({f"iter{it}_align_call_wall_us": wall(lambda: m.keyframe_align(snap, oa, R0, t0), reps),
                    f"iter{it}_align_call_wall_us_profiler_on": wall_prof,
                    f"iter{it}_pose_call_wall_us": wall(lambda: m.keyframe_pose(snap, op), reps),
                    f"iter{it}_align_status": a.status, f"iter{it}_align_used": a.used, f"iter{it}_pose_status": p.status,
                    f"iter{it}_pose_candidates": p.candidates, f"iter{it}_pose_used": p.used})
        if it == 8:
            out.update({k + "_us": round(prof[k][0], 2) for k in ("k_kf_align_sums", "k_kf_pose_step")})
    ctx.profile(True, only="k_kf_snapshot_normals")
    ctx.profile_reset()
    for _ in range(min(reps, 32)):
        snap.add_normals(mk)
    mk.size()
    snap.download()  # (waits for the track stream)
    out["k_kf_snapshot_normals_us"] = round(ctx.profile_read()["k_kf_snapshot_normals"][0], 2)
    ctx.profile(False)
    snap.release()
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
    snap.add_normals(maps[2])
    for k in range(2, 9):
        ctx.track_pair(maps[k], maps[k + 1])
    P = maps[9].keyframe_pose(snap)
    time_align(B, ctx, snap, maps[8], maps[9], args.reps, "640x480 bench stream, map 7 pairs behind its keyframe, guess = the chain's pose",
               (np.array(P.R), np.array(P.t)))
    ctx.close()
    small, qcam = synth.render_stream(576, 475, 3)
    big = np.ascontiguousarray(np.kron(small, np.ones((1, 4, 4), np.uint8)))
    H, W = big.shape[1:]
    ctx = B.Context(B.default_params(H, W, fm=qcam.fm * 4, cx=qcam.cx * 4 + 1.5, cy=qcam.cy * 4 + 1.5, keylines_ref=60000, keylines_max=65536))
    mk, m, spare = (ctx.detect_u8(big[i], i * 50000) for i in range(3))
    kf = mk.keylines()
    rng = np.random.default_rng(1)
    kf["matches"] = 3
    kf["rho"] = rng.uniform(0.2, 2.0, len(kf)).astype(np.float32)
    kf["sigma_rho"] = (0.05 * kf["rho"]).astype(np.float32)
    mk.upload(kf)
    snap = mk.keyframe_snapshot()
    snap.add_normals(mk)
    # the chain for the pose entry: ids written on the device by marking the current map (keyline i continues keyframe keyline i);
    # its keylines stay detection's, which the alignment asks for
    m.mark_keyframe()
    time_align(B, ctx, snap, spare, m, args.reps, f"{W}x{H}, keylines_max 65536, a detected map against a 65 536-keyline snapshot, identity guess")
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
    rates = {"pose": [], "align": []}
    status = {}
    for _ in range(args.rounds):
        for kind in ("pose", "align"):
            path = os.path.join(d, kind + ".txt")
            r = subprocess.run(base + ["--kf-" + kind, path], capture_output=True, text=True, timeout=300)
            m = re.search(r"= (\d+) frames/s", r.stderr)
            if r.returncode != 0 or not m:
                print(json.dumps(dict(what="host class", kind=kind, rc=r.returncode, stderr=r.stderr[-400:])), flush=True)
                return
            rates[kind].append(int(m.group(1)))
            st = [int(line.split()[1]) for line in open(path)]
            status[kind] = {s: st.count(s) for s in (0, 2, 3)}
    med = {k: float(np.median(v)) for k, v in rates.items()}
    print(json.dumps(dict(what="rebvio::Rebvio on the 640x480 bench stream (rebvio_replay), frames/s first to last record", frames=n,
                          with_kf_pose=rates["pose"], with_kf_align=rates["align"], median_pose=med["pose"], median_align=med["align"],
                          ratio=round(med["align"] / med["pose"], 4), status_pose=status["pose"], status_align=status["align"])), flush=True)


def basin(args):
    import torch  # noqa: F401
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import params_for
    from kf_align_ref import craft_against, craft_kf_keylines, np_kf_align, offset_guess, unit_of
    from kf_pose_ref import pose_err
    from rebvio_amd import backend as B
    from rebvio_amd import synth
    frames, cam = synth.render_stream(160, 120, 3)
    ctx = B.Context(params_for(B, cam, keylines_ref=1200, keylines_max=1601, global_min_matches_threshold=1))
    mk, mc = [ctx.detect_u8(frames[1 + k], k * 50000) for k in range(2)]
    kl = mc.keylines()
    ids, dists = mc.distance_field()
    camt = (ctx.p.fm, ctx.p.cx, ctx.p.cy, ctx.rows, ctx.cols)
    A = craft_against(kl, ids, dists, 1, camt)
    base = mk.keylines()
    base["matches"] = 0
    mk.upload(craft_kf_keylines(base, A, min(len(A["prs4"]), len(base))))
    bare = mk.keyframe_snapshot()
    snap = mk.keyframe_snapshot()
    snap.add_normals(mk)
    prs4, mt = snap.download()
    cur = (np.ascontiguousarray(kl["pos"]), unit_of(kl), ids.reshape(-1), dists.reshape(-1))
    for off in (0.002, 0.005, 0.01, 0.02, 0.03, 0.05):
        R0, t0 = offset_guess(off, 4 * off)
        row = dict(what="basin", rot_rad=off, trans=4 * off, kf_size=len(prs4))
        for name, s, nrm in (("normals", snap, snap.normals()), ("no_normals", bare, None)):
            ref = np_kf_align(camt, prs4, mt, nrm, *cur, R0, t0)
            got = mc.keyframe_align(s, None, R0, t0)
            row.update({name + "_err_np": float(f"{pose_err(ref['R'], ref['t']):.3g}"), name + "_err_device": float(f"{pose_err(got.R, got.t):.3g}"),
                        name + "_used": got.used, name + "_status": got.status,
                        name + "_dev_vs_np": float(f"{pose_err(got.R, got.t, ref['R'], ref['t']):.3g}"), name + "_guard": float(f"{ref['guard']:.3g}")})
        print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernels", "host", "basin"])
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    if "kernels" in a.what:
        kernels(a)
    if "host" in a.what:
        host(a)
    if "basin" in a.what:
        basin(a)
