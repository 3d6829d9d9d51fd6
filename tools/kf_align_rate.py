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

  many      rebvio_hip_map_keyframe_align_many on the first map of `kernels`: the wall time of ONE call with n = 1, 4,
            16 and 64 hypotheses (the same 16 000-keyline snapshot, seeded guesses around the chain's pose, max_iter 8) against n
            back-to-back rebvio_hip_map_keyframe_align calls on the same guesses, alternating in the same process, `--rounds` times
            `--reps` calls each (medians); device time per launch of k_kf_align_sums_many and k_kf_pose_step_many at every n
  multistart  the basin scene again: 13 starts at 0.03 rad / 0.12 units around the guess (rebvio_hip_kf_hypotheses_around), best by
            inliers (rebvio_hip_kf_align_best, min_inliers 12), device and restatement
  window    rebvio_replay on the bench stream with --kf-align alone and with --kf-window 4 and 15 next to it (a keyframe every 10
            records), processes alternating, `--rounds` times each; --parent-exe: another build's rebvio_replay (--kf-align alone) in
            the same rotation

    tools/kf_align_rate.py [kernels] [host] [basin] [many] [multistart] [window] [--frames N] [--rounds R] [--reps K] [--parent-exe PATH]"""
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


def bench_map():
    """the first map of `kernels`: (B, ctx, snapshot with normals, the map 7 pairs behind it, the chain's pose)"""
    import torch  # noqa: F401
    from rebvio_amd import backend as B
    from rebvio_amd import synth
    frames, cam = synth.render_stream(640, 480, 10)
    ctx = B.Context(B.default_params(480, 640, fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=15000, keylines_max=16000))
    maps = [ctx.detect_u8(frames[i], i * 50000) for i in range(10)]
    for k in range(2):
        ctx.track_pair(maps[k], maps[k + 1])
    maps[2].mark_keyframe()
    snap = maps[2].keyframe_snapshot()
    snap.add_normals(maps[2])
    for k in range(2, 9):
        ctx.track_pair(maps[k], maps[k + 1])
    return B, ctx, snap, maps[9], maps[9].keyframe_pose(snap)


def many(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from support import rodrigues
    B, ctx, snap, m, P = bench_map()
    R, t = np.array(P.R).reshape(3, 3), np.array(P.t)
    rng = np.random.default_rng(1)
    guesses = [(rodrigues(rng.uniform(-0.003, 0.003, 3)) @ R, t + rng.uniform(-0.01, 0.01, 3)) for _ in range(64)]
    opts = B.default_kf_align_opts(ctx, max_iter=8)
    for n in (1, 4, 16, 64):
        hyps = [B.kf_hypothesis(snap, *g) for g in guesses[:n]]
        batched = lambda: m.keyframe_align_many(hyps, opts)

        def singles():
            for R0, t0 in guesses[:n]:
                m.keyframe_align(snap, opts, R0, t0)
        res = batched()  # warm: scratch allocated
        singles()
        same = all(bytes(r.pose) == bytes(m.keyframe_align(snap, opts, *g)) for r, g in zip(res, guesses))
        wb, ws = [], []
        for _ in range(args.rounds):
            wb.append(wall(batched, args.reps))
            ws.append(wall(singles, max(1, args.reps // n)))
        ctx.profile(True, only="k_kf_*")
        ctx.profile_reset()
        for _ in range(min(args.reps, 32)):
            batched()
        prof = ctx.profile_read()
        ctx.profile_reset()
        singles()
        prof1 = ctx.profile_read()
        ctx.profile(False)
        mb, ms = float(np.median(wb)), float(np.median(ws))
        print(json.dumps(dict(what="align_many: one call against n single calls, 640x480 bench stream, 16 000-keyline snapshot, max_iter 8", n=n,
                              kf_size=len(snap.download()[0]), keylines=m.size(), reps=args.reps, rounds=args.rounds,
                              many_call_wall_us=wb, n_single_calls_wall_us=ws, median_many_us=mb, median_singles_us=ms,
                              ratio=round(mb / ms, 4), bit_identical=same, statuses=sorted({r.pose.status for r in res}),
                              k_kf_align_sums_many_us=round(prof["k_kf_align_sums_many"][0], 2),
                              k_kf_pose_step_many_us=round(prof["k_kf_pose_step_many"][0], 2),
                              k_kf_align_sums_us=round(prof1["k_kf_align_sums"][0], 2), k_kf_pose_step_us=round(prof1["k_kf_pose_step"][0], 2))),
              flush=True)
    snap.release()
    ctx.close()


def multistart(args):
    import torch  # noqa: F401
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import params_for
    from kf_align_many_ref import ROT_STEP, TRANS_STEP, hyp_Rt, np_inliers, py_best
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
    snap = mk.keyframe_snapshot()
    snap.add_normals(mk)
    prs4, mt = snap.download()
    D = (camt, prs4, mt, snap.normals(), np.ascontiguousarray(kl["pos"]), unit_of(kl), ids.reshape(-1), dists.reshape(-1))
    for off in (0.002, 0.005, 0.01, 0.02, 0.03, 0.05):
        R0, t0 = offset_guess(off, 4 * off)
        hyps = B.kf_hypotheses_around(snap, R0, t0, ROT_STEP, TRANS_STEP)
        res = mc.keyframe_align_many(hyps)
        best = B.kf_align_best(res, 12)
        refs, rows, guard = [], [], np.inf
        for h in hyps:
            ref = np_kf_align(*D, *hyp_Rt(h))
            inl, used, g = np_inliers(*D, ref["R"], ref["t"])
            guard = min(guard, ref["guard"], *g.values())
            refs.append(ref)
            rows.append((ref["status"], inl, ref["cost"]))
        nb = py_best(rows, 12)
        row = dict(what="multistart: 13 starts at 0.03 / 0.12, best by inliers", rot_rad=off, trans=4 * off, kf_size=len(prs4),
                   centre_err_device=float(f"{pose_err(res[0].pose.R, res[0].pose.t):.3g}"), centre_inliers=res[0].inliers,
                   best_device=best, best_np=nb, inliers_device=[r.inliers for r in res], inliers_np=[r[1] for r in rows],
                   guard=float(f"{guard:.3g}"))
        if best >= 0:
            row.update(best_err_device=float(f"{pose_err(res[best].pose.R, res[best].pose.t):.3g}"), best_inliers=res[best].inliers,
                       best_used=res[best].pose.used)
        if nb >= 0:
            row.update(best_err_np=float(f"{pose_err(refs[nb]['R'], refs[nb]['t']):.3g}"))
        if best >= 0 and best == nb:
            row.update(best_dev_vs_np=float(f"{pose_err(res[best].pose.R, res[best].pose.t, refs[nb]['R'], refs[nb]['t']):.3g}"))
        print(json.dumps(row), flush=True)
    snap.release()
    ctx.close()


def window(args):
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
    tail = ["--raw", os.path.join(d, "f.u8"), "--size", "640", "480", "--imu", os.path.join(d, "imu.bin"), "--camera", str(cam.fm),
            str(cam.cx), str(cam.cy), "--keylines", "15000", "16000", "--out", os.path.join(d, "o.txt"), "--kf-align", os.path.join(d, "a.txt")]
    kinds = {"align": [exe] + tail, "window4": [exe] + tail + ["--kf-window", "4", os.path.join(d, "w.txt")],
             "window15": [exe] + tail + ["--kf-window", "15", os.path.join(d, "w.txt")]}
    if args.parent_exe:
        kinds["parent_align"] = [args.parent_exe] + tail
    rates = {k: [] for k in kinds}
    lines, poses = {}, {}
    for _ in range(args.rounds):
        for kind, cmd in kinds.items():
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            m = re.search(r"= (\d+) frames/s", r.stderr)
            if r.returncode != 0 or not m:
                print(json.dumps(dict(what="window", kind=kind, rc=r.returncode, stderr=r.stderr[-400:])), flush=True)
                return
            rates[kind].append(int(m.group(1)))
            poses[kind] = open(os.path.join(d, "a.txt")).read()
            if kind.startswith("window"):
                per = {}
                for line in open(os.path.join(d, "w.txt")):
                    per[line.split()[0]] = per.get(line.split()[0], 0) + 1
                lines[kind] = dict(lines=sum(per.values()), records=len(per), most_per_record=max(per.values()))
    med = {k: float(np.median(v)) for k, v in rates.items()}
    out = dict(what="rebvio::Rebvio on the 640x480 bench stream (rebvio_replay), frames/s first to last record, --kf-align with a window", frames=n,
               rates=rates, medians=med, window4_over_align=round(med["window4"] / med["align"], 4),
               window15_over_align=round(med["window15"] / med["align"], 4), window_files=lines,
               pose_files_equal=all(p == poses["align"] for p in poses.values()))
    if args.parent_exe:
        out["align_over_parent_align"] = round(med["align"] / med["parent_align"], 4)
    print(json.dumps(out), flush=True)


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
    ap.add_argument("--parent-exe", default="")
    a = ap.parse_args()
    if "kernels" in a.what:
        kernels(a)
    if "host" in a.what:
        host(a)
    if "basin" in a.what:
        basin(a)
    if "many" in a.what:
        many(a)
    if "multistart" in a.what:
        multistart(a)
    if "window" in a.what:
        window(a)
