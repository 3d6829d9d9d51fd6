"""Detection masks (rebvio_hip_set_detection_mask and the *_masked_device entries): a masked pixel is skipped in buildEdgeMap
(edge_detector.cpp:73-121) exactly like one that fails the magnitude test. The expected masked map is built (support.masked_map)
from the oracle's UNMASKED map at the same threshold: drop the keylines whose pixel is masked, truncate at keylines_max, chain with
a numpy statement of joinEdges, threshold with one of tuneThreshold. Every comparison is bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import params_for
from support import B, host_lib  # noqa: F401
from support import (EUROC_D, INC, KW_C2, ROOT, assert_keylines_equal, assert_map, bits_equal, c2_order, masked_map, rec, record_words,
                     same_records)

pytestmark = pytest.mark.gpu

KMAX_ALL = 65536   # the oracle's budget: every candidate of a 640x480 frame


def blocky_mask(H, W, seed, block=16, p=0.6):
    rng = np.random.default_rng(seed)
    m = np.kron(rng.random((H // block + 1, W // block + 1)) < p, np.ones((block, block), bool))[:H, :W]
    return m.astype(np.uint8) * np.uint8(rng.integers(1, 256))   # any non-zero byte means "detect here"


def noise_mask(H, W, seed, p=0.7):
    return (np.random.default_rng(seed).random((H, W)) < p).astype(np.uint8)


def bottom_third_masked(H, W):
    m = np.ones((H, W), np.uint8)
    m[H - H // 3:] = 0
    return m


# ---- 1. against the oracle, threshold fixed --------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "radtan"])
@pytest.mark.parametrize("kind", ["static", "per-frame"])
@pytest.mark.parametrize("kmax", [16000, 3000])
def test_masked_map_equals_the_oracle_map_with_masked_pixels_dropped(orc_mod, B, c2_stream, lens, kind, kmax):
    frames, cam = c2_stream
    H, W = cam.height, cam.width
    orc = orc_mod.Oracle(params_for(orc_mod, cam, keylines_max=KMAX_ALL, gain=0.0))
    ctx = B.Context(params_for(B, cam, keylines_ref=kmax, keylines_max=kmax, gain=0.0))
    if lens:
        ctx.set_undistort(cam.fm, cam.fm, cam.cx, cam.cy, EUROC_D)
    masks = [blocky_mask(H, W, 1), noise_mask(H, W, 2), bottom_third_masked(H, W), blocky_mask(H, W, 3, block=5, p=0.3)]
    dev = ctx.upload_frames(frames)
    mdev = ctx.upload_frames(np.stack(masks))
    auto = np.float32(ctx.p.threshold)
    truncated = 0
    for i in range(len(frames)):
        keep = masks[i % len(masks)]
        if lens:
            om = orc.detect(orc.front_end_u8(frames[i], cam.fm, cam.fm, cam.cx, cam.cy, EUROC_D), i * 50000)
        else:
            om = orc.detect_u8(frames[i], i * 50000)
        want = masked_map(om, H, W, keep, kmax, auto)
        truncated += int(len(want[0]) == kmax)
        if kind == "static":
            ctx.set_detection_mask(keep)
            gm = ctx.detect_u8_host(frames[i], i * 50000) if lens else ctx.detect_u8(frames[i], i * 50000)
        else:
            gm = ctx.detect_px_masked_device(dev + i * H * W, B.PX_GRAY8, mdev + (i % len(masks)) * H * W, i * 50000)
        assert_map(want, gm, f"frame {i}")
        assert len(want[0]) > 300 and len(want[0]) < om.size()
        thr, auto_dev, cnt = ctx.detector_state()
        assert cnt == len(want[0]) and bits_equal(np.float32(auto_dev), want[2])
        auto = want[2]
        gm.release()
    if kmax == 3000:
        assert truncated == len(frames)   # truncation counted behind masked candidates on every frame
    ctx.close()


# ---- 2. the threshold servo on the masked counts -------------------------------------------------------------------------
def test_threshold_servo_follows_the_masked_keyline_count(orc_mod, B, c2_stream):
    frames, cam = c2_stream
    H, W = cam.height, cam.width
    kref, kmax, gain = 6000, 16000, np.float32(2e-6)
    ctx = B.Context(params_for(B, cam, keylines_ref=kref, keylines_max=kmax, gain=float(gain)))
    p = ctx.p
    keep = blocky_mask(H, W, 7)
    ctx.set_detection_mask(keep)
    thr, auto, count = np.float32(p.threshold), np.float32(p.threshold), 0
    thrs = []
    for i in range(len(frames)):
        # EdgeDetector::detect (edge_detector.cpp:33-36) in float32
        thr = np.float32(thr - np.float32(gain * np.float32(kref - count)))
        thr = min(max(thr, np.float32(p.min_threshold)), np.float32(p.max_threshold))
        thrs.append(thr)
        orc = orc_mod.Oracle(params_for(orc_mod, cam, keylines_max=KMAX_ALL, gain=0.0, threshold=float(thr)))
        want = masked_map(orc.detect_u8(frames[i], i * 50000), H, W, keep, kmax, auto)
        gm = ctx.detect_u8(frames[i], i * 50000)
        assert_map(want, gm, f"frame {i}")
        t_dev, a_dev, c_dev = ctx.detector_state()
        assert bits_equal(np.float32(t_dev), thr), (i, t_dev, thr)
        assert c_dev == len(want[0]) and bits_equal(np.float32(a_dev), want[2])
        count, auto = len(want[0]), want[2]
        gm.release()
    assert len(set(thrs)) >= 4, thrs     # the servo moved
    ctx.close()


# ---- 3 / 4. all-ones masks, and the streaming driver against the per-pair API --------------------------------------------------


def _pairs(B, cam, frames, order, static=None, per_frame=None):
    """per-pair API: masked detect + rebvio_hip_track_pair; every record as words (+ the new map's size), the last map's keylines"""
    ctx = B.Context(params_for(B, cam, **KW_C2))
    npx = cam.width * cam.height
    dev = ctx.upload_frames(frames)
    if static is not None:
        ctx.set_detection_mask(static)
    mdev = ctx.upload_frames(per_frame[None]) if per_frame is not None else None
    maps, recs = [], []
    for k, i in enumerate(order):
        if mdev is None:
            maps.append(ctx.detect_u8_device(dev + int(i) * npx, k * 50000))
        else:
            maps.append(ctx.detect_px_masked_device(dev + int(i) * npx, B.PX_GRAY8, mdev, k * 50000))
        if len(maps) > 2:
            maps.pop(0).release()
        if k:
            recs.append(rec(ctx.track_pair(maps[0], maps[1]), maps[1].size()))
    kl = maps[-1].keylines()
    ctx.close()
    return recs, kl


def _stream(B, cam, frames, order, static=None, per_frame=None):
    ctx = B.Context(params_for(B, cam, **KW_C2))
    npx = cam.width * cam.height
    dev = ctx.upload_frames(frames)
    if static is not None:
        ctx.set_detection_mask(static)
    mdev = ctx.upload_frames(per_frame[None]) if per_frame is not None else None
    recs = []
    for k, i in enumerate(order):
        if mdev is None:
            out, n = ctx.push_frame_u8_device(dev + int(i) * npx, k * 50000)
        else:
            out, n = ctx.push_frame_px_masked_device(dev + int(i) * npx, B.PX_GRAY8, mdev, k * 50000)
        if out.status >= 0:
            recs.append(rec(out, n))
    recs.extend(rec(o, n) for o, n in ctx.flush())
    state = ctx.detector_state()
    ctx.close()
    return recs, state


def test_all_ones_mask_equals_no_mask(B, c2_stream):
    frames, cam = c2_stream
    H, W = cam.height, cam.width
    order = c2_order()
    ones = np.full((H, W), 255, np.uint8)
    want, kl = _pairs(B, cam, frames, order)
    for kw in (dict(static=ones), dict(per_frame=ones), dict(static=ones, per_frame=ones)):
        got, kg = _pairs(B, cam, frames, order, **kw)
        same_records(want, got, f"per-pair {list(kw)}")
        assert_keylines_equal(kl, kg, what=f"per-pair {list(kw)}")
    want_s, st = _stream(B, cam, frames, order)
    same_records(want, want_s, "per-pair vs stream, no mask")
    for kw in (dict(static=ones), dict(per_frame=ones)):
        got, sg = _stream(B, cam, frames, order, **kw)
        same_records(want_s, got, f"stream {list(kw)}")
        assert all(bits_equal(np.float32(a), np.float32(b)) for a, b in zip(st, sg))
    assert want[-1][-1] > 1000 and any(w[0] != 0 for w in want)
    # a 4-lane batch: static all-ones masks on lanes 0 / 1, per-frame ones on lanes 2 / 3, against a batch without masks
    from rebvio_amd import synth
    L = 4
    streams = [synth.render_stream(W, H, 8, stream_id=l)[0] for l in range(L)]
    a = _batch(B, cam, streams, order)
    b = _batch(B, cam, streams, order, static=[ones, ones, None, None], per_frame=[None, None, ones, ones])
    for l in range(L):
        same_records(a[l], b[l], f"batch lane {l}")


def test_streaming_driver_with_masks_equals_the_per_pair_api(B, c2_stream):
    frames, cam = c2_stream
    H, W = cam.height, cam.width
    order = c2_order()
    for kw in (dict(static=blocky_mask(H, W, 4)), dict(per_frame=noise_mask(H, W, 5)),
               dict(static=bottom_third_masked(H, W), per_frame=blocky_mask(H, W, 6))):
        want, _ = _pairs(B, cam, frames, order, **kw)
        got, _ = _stream(B, cam, frames, order, **kw)
        same_records(want, got, list(kw))
        assert want[-1][-1] > 500


# ---- 5. per-frame masks equal the same static mask; the two combine as their AND ----------------------------------------------
def test_per_frame_mask_equals_static_mask_and_they_combine_as_and(B, c2_stream):
    frames, cam = c2_stream
    H, W = cam.height, cam.width
    order = c2_order()
    m1, m2 = blocky_mask(H, W, 8), noise_mask(H, W, 9, p=0.8)
    s, _ = _stream(B, cam, frames, order, static=m1)
    f, _ = _stream(B, cam, frames, order, per_frame=m1)
    same_records(s, f, "static vs per-frame")
    both = (m1 != 0) & (m2 != 0)
    a, _ = _stream(B, cam, frames, order, static=m1, per_frame=m2)
    b, _ = _stream(B, cam, frames, order, static=both.astype(np.uint8))
    c, _ = _stream(B, cam, frames, order, static=m2, per_frame=m1)
    same_records(a, b, "static m1 + per-frame m2 vs static (m1 & m2)")
    same_records(a, c, "the two kinds swapped")
    none, _ = _stream(B, cam, frames, order)
    assert not all(np.array_equal(x, y) for x, y in zip(none, s))      # the mask matters
    assert a[-1][-1] < s[-1][-1]


# ---- 6. batch lanes with different masks against stand-alone contexts ------------------------------------------------------------
def _batch(B, cam, streams, order, static=None, per_frame=None, lens=False):
    L = len(streams)
    H, W = cam.height, cam.width
    b = B.Batch(params_for(B, cam, **KW_C2), L)
    if lens:
        for ctx in b.lanes:
            ctx.set_undistort(cam.fm, cam.fm, cam.cx, cam.cy, EUROC_D)
    devs = [b.lanes[l].upload_frames(streams[l]) for l in range(L)]
    for l in range(L):
        if static is not None and static[l] is not None:
            b.lanes[l].set_detection_mask(static[l])
    mdev = [b.lanes[l].upload_frames(per_frame[l][None]) if per_frame is not None and per_frame[l] is not None else None
            for l in range(L)]
    recs = [[] for _ in range(L)]

    def take(outs, ns):
        for l in range(L):
            if outs[l].status >= 0:
                recs[l].append(rec(outs[l], ns[l]))

    for k, i in enumerate(order):
        fr = [devs[l] + int(i) * H * W for l in range(L)]
        if per_frame is None:
            take(*b.push_u8_device(fr, k * 50000))
        else:
            take(*b.push_px_masked_device(fr, B.PX_GRAY8, mdev, k * 50000))
    for outs, ns in b.flush():
        take(outs, ns)
    b.close()
    return recs


@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "radtan"])
def test_batch_lanes_with_different_masks_equal_stand_alone_contexts(B, lens):
    from rebvio_amd import synth
    W, H, L = 640, 480, 4
    streams = [synth.render_stream(W, H, 8, stream_id=l)[0] for l in range(L)]
    cam = synth.render_stream(W, H, 1)[1]
    order = c2_order()
    static = [blocky_mask(H, W, 10), None, bottom_third_masked(H, W), None]
    per_frame = [None, noise_mask(H, W, 11), blocky_mask(H, W, 12), None]
    got = _batch(B, cam, streams, order, static, per_frame, lens)
    for l in range(L):
        ctx = B.Context(params_for(B, cam, **KW_C2))
        if lens:
            ctx.set_undistort(cam.fm, cam.fm, cam.cx, cam.cy, EUROC_D)
        dev = ctx.upload_frames(streams[l])
        if static[l] is not None:
            ctx.set_detection_mask(static[l])
        mdev = ctx.upload_frames(per_frame[l][None]) if per_frame[l] is not None else None
        want = []
        for k, i in enumerate(order):
            fa = dev + int(i) * H * W
            out, n = (ctx.push_frame_px_masked_device(fa, B.PX_GRAY8, mdev, k * 50000) if mdev is not None
                      else ctx.push_frame_u8_device(fa, k * 50000))
            if out.status >= 0:
                want.append(rec(out, n))
        want.extend(rec(o, n) for o, n in ctx.flush())
        ctx.close()
        same_records(want, got[l], f"lane {l}")
        assert len(want) == len(order) - 1 and want[-1][-1] > 500


# ---- 7. a static mask changed in the middle of a stream ----------------------------------------------------------------------
def test_static_mask_change_applies_from_the_next_frame_on(B, c2_stream):
    """Frames pushed before set_detection_mask keep the old mask (the call rewrites the device copy only after their candidate
    kernels have run), frames pushed after it get the new one: the same records as per-frame masks switched at that frame."""
    frames, cam = c2_stream
    H, W = cam.height, cam.width
    order = c2_order()
    npx = H * W
    m_old, m_new, switch = blocky_mask(H, W, 13), noise_mask(H, W, 14), 7

    def run(static):
        ctx = B.Context(params_for(B, cam, **KW_C2))
        dev = ctx.upload_frames(frames)
        mdev = ctx.upload_frames(np.stack([m_old, m_new]))
        recs = []
        if static:
            ctx.set_detection_mask(m_old)
        for k, i in enumerate(order):
            if static:
                if k == switch:
                    ctx.set_detection_mask(m_new)
                out, n = ctx.push_frame_u8_device(dev + int(i) * npx, k * 50000)
            else:
                out, n = ctx.push_frame_px_masked_device(dev + int(i) * npx, B.PX_GRAY8, mdev + (k >= switch) * npx, k * 50000)
            if out.status >= 0:
                recs.append(rec(out, n))
        recs.extend(rec(o, n) for o, n in ctx.flush())
        ctx.close()
        return recs

    same_records(run(False), run(True), "static mask switched at frame 7")
    # and in a batch lane: picked up by the next push
    from rebvio_amd import synth
    streams = [synth.render_stream(W, H, 8, stream_id=l)[0] for l in range(2)]

    def run_batch(static):
        b = B.Batch(params_for(B, cam, **KW_C2), 2)
        devs = [b.lanes[l].upload_frames(streams[l]) for l in range(2)]
        mdev = [b.lanes[l].upload_frames(np.stack([m_old, m_new])) for l in range(2)]
        recs = [[], []]
        if static:
            b.lanes[1].set_detection_mask(m_old)
        for k, i in enumerate(order):
            fr = [devs[l] + int(i) * npx for l in range(2)]
            if static:
                if k == switch:
                    b.lanes[1].set_detection_mask(m_new)
                outs, ns = b.push_u8_device(fr, k * 50000)
            else:
                outs, ns = b.push_px_masked_device(fr, B.PX_GRAY8, [None, mdev[1] + (k >= switch) * npx], k * 50000)
            for l in range(2):
                if outs[l].status >= 0:
                    recs[l].append(rec(outs[l], ns[l]))
        for outs, ns in b.flush():
            for l in range(2):
                recs[l].append(rec(outs[l], ns[l]))
        b.close()
        return recs

    a, c = run_batch(False), run_batch(True)
    for l in range(2):
        same_records(a[l], c[l], f"batch lane {l}")


# ---- 8. argument refusals ----------------------------------------------------------------------------------------------------
def test_masked_entries_refuse_bad_arguments_before_queueing(B, c2_stream):
    import ctypes as C
    frames, cam = c2_stream
    H, W = cam.height, cam.width
    L = B.lib()
    ctx = B.Context(params_for(B, cam, **KW_C2))
    dev = C.c_void_p(ctx.upload_frames(frames[:1]))
    mdev = C.c_void_p(ctx.upload_frames(np.ones((1, H, W), np.uint8)))
    h = C.c_void_p()
    out = B.PairOut()
    n = C.c_int()

    def refused(rc, words):
        msg = L.rebvio_hip_last_error().decode()
        assert rc == -3 and all(w in msg for w in words), (rc, msg)

    refused(L.rebvio_hip_detect_px_masked_device(ctx.h, None, 0, mdev, 0, C.byref(h)), ["null frame"])
    refused(L.rebvio_hip_detect_px_masked_device(ctx.h, dev, 0, None, 0, C.byref(h)), ["null mask"])
    refused(L.rebvio_hip_detect_px_masked_device(ctx.h, dev, 9, mdev, 0, C.byref(h)), ["unknown pixel format"])
    refused(L.rebvio_hip_push_frame_px_masked_device(ctx.h, None, 0, mdev, 0, C.byref(out), C.byref(n)), ["null frame"])
    refused(L.rebvio_hip_push_frame_px_masked_device(ctx.h, dev, 0, None, 0, C.byref(out), C.byref(n)), ["null mask"])
    refused(L.rebvio_hip_push_frame_px_masked_device(ctx.h, dev, -1, mdev, 0, C.byref(out), C.byref(n)), ["unknown pixel format"])
    host = np.ones((H, W), np.uint8)
    refused(L.rebvio_hip_set_detection_mask(ctx.h, host.ctypes.data_as(C.c_void_p), W - 1), ["pitch_bytes"])
    b = B.Batch(params_for(B, cam, **KW_C2), 2)
    bdev = [b.lanes[l].upload_frames(frames[:1]) for l in range(2)]
    bm = (C.c_void_p * 2)(None, None)
    refused(L.rebvio_hip_batch_push_px_masked_device(b.h, (C.c_void_p * 2)(bdev[0], None), 0, bm, 0, b._out, b._n), ["null frame"])
    refused(L.rebvio_hip_batch_push_px_masked_device(b.h, (C.c_void_p * 2)(*bdev), 7, bm, 0, b._out, b._n), ["unknown pixel format"])
    refused(L.rebvio_hip_batch_push_px_masked_device(b.h, (C.c_void_p * 2)(*bdev), 0, None, 0, b._out, b._n), ["null mask array"])
    # the Python layer: shape checks
    with pytest.raises(ValueError):
        ctx.set_detection_mask(np.ones((H, W + 1)))
    # nothing was queued: the context and the batch still run, and a stream still matches one that never saw a refusal
    outs, _ = b.push_px_masked_device(bdev, B.PX_GRAY8, [None, None], 0)
    b.close()
    ref = B.Context(params_for(B, cam, **KW_C2))
    rdev = ref.upload_frames(frames)
    cdev = ctx.upload_frames(frames)
    for k in range(4):
        a, _ = ref.push_frame_u8_device(rdev + k * H * W, k * 50000)
        c, _ = ctx.push_frame_px_masked_device(cdev + k * H * W, B.PX_GRAY8, mdev.value, k * 50000)
        assert np.array_equal(record_words(a), record_words(c)), k
    ra, rc_ = ref.flush(), ctx.flush()
    assert len(ra) == len(rc_) and all(np.array_equal(record_words(x[0]), record_words(y[0])) for x, y in zip(ra, rc_))
    ref.close()
    ctx.close()


# ---- torch tensors as frames and masks -----------------------------------------------------------------------------------------
def test_torch_tensors_as_per_frame_masks(B, c2_stream):
    import torch
    frames, cam = c2_stream
    H, W = cam.height, cam.width
    order = c2_order()
    m = blocky_mask(H, W, 15)
    want, _ = _stream(B, cam, frames, order, static=m)
    ctx = B.Context(params_for(B, cam, **KW_C2))
    ft = torch.from_numpy(frames).to("cuda:0")
    mt = torch.from_numpy(m != 0).to("cuda:0")          # bool
    got = []
    for k, i in enumerate(order):
        out, n = ctx.push_frame_px_masked_device(ft[int(i)], B.PX_GRAY8, mt, k * 50000)
        if out.status >= 0:
            got.append(rec(out, n))
    got.extend(rec(o, n) for o, n in ctx.flush())
    with pytest.raises(TypeError):
        ctx.detect_px_masked_device(ft[0], B.PX_GRAY8, mt.float())
    with pytest.raises(ValueError):
        ctx.detect_px_masked_device(ft[0], B.PX_GRAY8, mt[:, :-1])
    ctx.close()
    same_records(want, got, "torch tensors")


# ---- 9 / 10. the C++ class and rebvio_replay ---------------------------------------------------------------------------------------


def test_cpp_rebvio_set_detection_mask(host_lib, tmp_path):
    """rebvio::Rebvio::setDetectionMask: an all-ones mask gives the odometry of no mask, byte for byte; a mask of the top half
    changes it and no keyline of any published edge map lies in the masked bottom half."""
    from rebvio_amd import synth
    n, W, H = 22, 320, 240
    grey, cam = synth.render_stream(W, H, n)
    scene = synth.make_scene(0)
    ts, gyro, acc = synth.imu_samples(scene, n, noise_seed=1)
    rec = np.zeros(len(ts), dtype=[("ts", "<i8"), ("gyro", "<f4", 3), ("acc", "<f4", 3)])
    rec["ts"], rec["gyro"], rec["acc"] = ts, gyro, acc
    rec.tofile(tmp_path / "imu.bin")
    grey.tofile(tmp_path / "grey.u8")
    exe = str(tmp_path / "detection_mask")
    subprocess.run(["g++", "-std=c++17", "-O1"] + INC + [os.path.join(ROOT, "tests", "cpp", "test_detection_mask.cpp"), "-o", exe,
                    "-L", host_lib, "-lrebvio", "-lrebvio_hip", f"-Wl,-rpath,{host_lib}", "-pthread"], check=True)

    def run(mode):
        r = subprocess.run([exe, mode, str(tmp_path / "grey.u8"), str(W), str(H), str(n), repr(cam.fm), repr(cam.cx), repr(cam.cy),
                            str(tmp_path / "imu.bin")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (mode, r.stdout[-1000:], r.stderr[-2000:])
        return r.stdout

    none, ones, half = run("none"), run("ones"), run("half")
    assert len(none.strip().splitlines()) == n - 1
    assert ones == none
    assert half != none


def test_replay_mask_flag_with_an_all_ones_png(host_lib, tmp_path):
    from pngutil import write_asl, write_png
    from rebvio_amd import synth
    n, W, H = 12, 320, 240
    grey, cam = synth.render_stream(W, H, n)
    scene = synth.make_scene(0)
    its, gyro, acc = synth.imu_samples(scene, n, noise_seed=1)
    ts = np.arange(n) * 50000 + 1000000
    write_asl(str(tmp_path / "mav0"), grey, ts, its + 1000000, gyro, acc)
    write_png(str(tmp_path / "ones.png"), np.full((H, W), 255, np.uint8))
    write_png(str(tmp_path / "small.png"), np.full((H - 1, W), 255, np.uint8))
    exe = os.path.join(host_lib, "rebvio_replay")
    common = ["--asl", str(tmp_path / "mav0"), "--camera", repr(cam.fm), repr(cam.cx), repr(cam.cy), "--keylines", "3000", "4000",
              "--min-matches", "50"]
    r1 = subprocess.run([exe] + common + ["--out", str(tmp_path / "plain.txt")], capture_output=True, text=True, timeout=300)
    r2 = subprocess.run([exe] + common + ["--mask", str(tmp_path / "ones.png"), "--out", str(tmp_path / "mask.txt")],
                        capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr[-1500:], r2.stderr[-1500:])
    a, b = (tmp_path / "plain.txt").read_bytes(), (tmp_path / "mask.txt").read_bytes()
    assert len(a.splitlines()) == n - 1 and a == b
    r3 = subprocess.run([exe] + common + ["--mask", str(tmp_path / "small.png"), "--out", str(tmp_path / "bad.txt")],
                        capture_output=True, text=True, timeout=300)
    assert r3.returncode == 1 and "mask" in r3.stderr and "320x239" in r3.stderr, r3.stderr[-500:]
