"""Colour and packed-YUV camera frames on the device (REBVIO_HIP_PX_*): every *_px entry against the grey path fed the grey frame
of the same pixels. The conversion is fused into the first scan pass (or the lens front end) and ends in the grey frame's fp32
values, so the comparison has no tolerance: every word of every pair record, every field of every keyline, the threshold
servo, the C++ class's odometry and edge-image frames, and rebvio_replay's odometry file, byte for byte.

Colour frames are built from the fixtures' grey streams: RGB channels = grey + a per-pixel chroma offset (clipped), and the
grey path gets formula(colour); YUYV / UYVY carry the grey frame as Y and random bytes as U / V."""
import os
import subprocess

import numpy as np
import pytest

from conftest import params_for
from support import B, host_lib  # noqa: F401
from support import (BGR8, BPP, EUROC_D, INC, KW_C2, NAMES, RGB8, RGBA8, ROOT, UYVY, YUYV, assert_keylines_equal, bits_equal, c2_order,
                     colourise, rec)

pytestmark = pytest.mark.gpu

FMTS = list(range(7))


@pytest.fixture(scope="module")
def px_stream(c2_stream):
    frames, cam = c2_stream
    return colourise(frames, 7), cam


def _padded(frame, pad, rng):
    """frame [H, W(, bpp)] as a view into rows of pitch W * bpp + pad whose padding holds garbage"""
    H, W = frame.shape[:2]
    bpp = 1 if frame.ndim == 2 else frame.shape[2]
    buf = rng.integers(0, 256, (H, W * bpp + pad), dtype=np.uint8)
    buf[:, :W * bpp] = frame.reshape(H, W * bpp)
    view = np.lib.stride_tricks.as_strided(buf, (H, W, bpp), (buf.strides[0], bpp, 1))
    return view if frame.ndim == 3 else view[..., 0], buf


def _stream_words(ctx, push, order):
    """push(k, i) for every frame, then flush: every record as words (+ keyline count), and the detector state at the end"""
    got = []
    for k, i in enumerate(order):
        out, n = push(k, int(i))
        if out.status >= 0:
            got.append(rec(out, n))
    got.extend(rec(o, n) for o, n in ctx.flush())
    return got, ctx.detector_state()


def _assert_same_stream(want, got, what):
    (rw, sw), (rg, sg) = want, got
    assert len(rw) == len(rg), (what, len(rw), len(rg))
    for k, (a, b) in enumerate(zip(rw, rg)):
        assert np.array_equal(a, b), (what, k, np.flatnonzero(a != b)[:8])
    assert all(bits_equal(np.float32(a), np.float32(b)) for a, b in zip(sw, sg)), (what, sw, sg)
    assert rw[-1][-1] > 1000 and any(w[0] != 0 for w in rw), what   # a real stream: keylines and motion


def _grey_stream(B, cam, grey, order, dist=None):
    ctx = B.Context(params_for(B, cam, **KW_C2))
    if dist is not None:
        ctx.set_undistort(cam.fm, cam.fm, cam.cx, cam.cy, dist)
    dev = ctx.upload_frames(grey)
    npx = cam.width * cam.height
    r = _stream_words(ctx, lambda k, i: ctx.push_frame_u8_device(dev + i * npx, k * 50000), order)
    ctx.close()
    return r


@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "radtan"])
@pytest.mark.parametrize("fmt", FMTS, ids=NAMES)
def test_streaming_device_frames_equal_the_grey_stream(B, px_stream, fmt, lens):
    """1 / 3: push_frame_px_device of each format == push_frame_u8_device of the grey frames, with and without a lens model
    (the front end's gather converts each of its four taps)."""
    px, cam = px_stream
    frames, grey = px[fmt]
    order = c2_order()
    dist = EUROC_D if lens else None
    want = _grey_stream(B, cam, grey, order, dist)
    ctx = B.Context(params_for(B, cam, **KW_C2))
    if lens:
        ctx.set_undistort(cam.fm, cam.fm, cam.cx, cam.cy, dist)
    dev = ctx.upload_frames(frames)
    fb = cam.width * cam.height * BPP[fmt]
    got = _stream_words(ctx, lambda k, i: ctx.push_frame_px_device(dev + i * fb, fmt, k * 50000), order)
    ctx.close()
    _assert_same_stream(want, got, NAMES[fmt])


@pytest.mark.parametrize("fmt", FMTS, ids=NAMES)
def test_streaming_host_frames_with_a_padded_pitch(B, px_stream, fmt):
    """2: push_frame_px of host frames whose rows are padded (garbage in the padding), the caller's buffer overwritten right
    after each push, == the grey stream."""
    px, cam = px_stream
    frames, grey = px[fmt]
    order = c2_order()
    want = _grey_stream(B, cam, grey, order)
    rng = np.random.default_rng(fmt)
    ctx = B.Context(params_for(B, cam, **KW_C2))

    def push(k, i):
        view, buf = _padded(frames[i], 12 + 4 * fmt, rng)
        r = ctx.push_frame_px(view, fmt, k * 50000)
        buf[:] = 0
        return r

    got = _stream_words(ctx, push, order)
    ctx.close()
    _assert_same_stream(want, got, NAMES[fmt])


@pytest.mark.parametrize("fmt", FMTS, ids=NAMES)
def test_front_end_px_equals_the_grey_front_end(B, px_stream, fmt):
    """3: front_end_px output bit-identical to front_end_u8 of the grey frame (barrel and pincushion lens: the latter reads the
    zero border), dense and with a padded pitch."""
    px, cam = px_stream
    frames, grey = px[fmt]
    ctx = B.Context(params_for(B, cam, **KW_C2))
    rng = np.random.default_rng(fmt)
    for D in (EUROC_D, [0.6, -0.1, 1e-3, -2e-3, 0.05]):
        ctx.set_undistort(cam.fm, cam.fm, cam.cx, cam.cy, D)
        for i in (0, 5):
            want = ctx.front_end_u8(grey[i])
            assert bits_equal(want, ctx.front_end_px(frames[i], fmt)), (NAMES[fmt], D, i)
            view, _ = _padded(frames[i], 20, rng)
            assert bits_equal(want, ctx.front_end_px(view, fmt)), (NAMES[fmt], D, i, "padded")
    ctx.close()


@pytest.mark.parametrize("shape", [(131, 67), (190, 143), (642, 480)], ids=["131x67", "190x143", "642x480"])
def test_detect_px_over_a_sequence_ragged_sizes(B, shape):
    """4: detect_px (host) and detect_px_device over a sequence: the keyline set, its order, every field and the threshold servo
    identical to detect_u8 / detect_u8_device of the grey frames. Ragged widths take the guarded element loads; YUYV / UYVY
    only on even widths."""
    from rebvio_amd import synth
    W, H = shape
    n = 5
    grey0, cam = synth.render_stream(W, H, n, stream_id=1)
    px = colourise(grey0, W)
    kw = dict(keylines_ref=3000, keylines_max=4000)
    for fmt in FMTS:
        if BPP[fmt] == 2 and W % 2:
            continue
        frames, grey = px[fmt]
        ref = B.Context(params_for(B, cam, **kw))
        ref_d = B.Context(params_for(B, cam, **kw))
        host = B.Context(params_for(B, cam, **kw))
        dev = B.Context(params_for(B, cam, **kw))
        gdev = ref_d.upload_frames(grey)
        cdev = dev.upload_frames(frames)
        fb = W * H * BPP[fmt]
        for i in range(n):
            a = ref.detect_u8_host(grey[i], i * 50000)
            b = host.detect_px(frames[i], fmt, i * 50000)
            c = ref_d.detect_u8_device(gdev + i * W * H, i * 50000)
            d = dev.detect_px_device(cdev + i * fb, fmt, i * 50000)
            ka = a.keylines()
            assert len(ka) > 50, (shape, NAMES[fmt], len(ka))
            assert_keylines_equal(ka, b.keylines(), what=f"{shape} {NAMES[fmt]} host frame {i}")
            assert_keylines_equal(c.keylines(), d.keylines(), what=f"{shape} {NAMES[fmt]} device frame {i}")
            assert_keylines_equal(ka, d.keylines(), what=f"{shape} {NAMES[fmt]} host/device frame {i}")
            assert a.threshold == b.threshold == c.threshold == d.threshold
            for m in (a, b, c, d):
                m.release()
        s = [ctx.detector_state() for ctx in (ref, host, ref_d, dev)]
        assert s[0] == s[1] and s[2] == s[3] and s[0] == s[2], (NAMES[fmt], s)
        for ctx in (ref, ref_d, host, dev):
            ctx.close()


@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "radtan"])
def test_format_changes_every_frame_host_and_device_mixed(B, px_stream, lens):
    """5: one stream, frame k in format k mod 7, host (padded) and device frames alternating: the records of the all-grey
    stream. A colour host frame after grey ones changes the device staging frame it goes through, mid-stream."""
    px, cam = px_stream
    order = c2_order()
    fmts = [k % 7 for k in range(len(order))]
    dist = EUROC_D if lens else None
    ref = B.Context(params_for(B, cam, **KW_C2))
    ctx = B.Context(params_for(B, cam, **KW_C2))
    if lens:
        ref.set_undistort(cam.fm, cam.fm, cam.cx, cam.cy, dist)
        ctx.set_undistort(cam.fm, cam.fm, cam.cx, cam.cy, dist)
    grey_seq = np.stack([px[f][1][i] for f, i in zip(fmts, order)])
    gdev = ref.upload_frames(grey_seq)
    npx = cam.width * cam.height
    want = _stream_words(ref, lambda k, i: ref.push_frame_u8_device(gdev + k * npx, k * 50000), order)
    devs = {f: ctx.upload_frames(px[f][0]) for f in FMTS}
    rng = np.random.default_rng(3)

    def push(k, i):
        f = fmts[k]
        if (k // 2) % 2:
            view, buf = _padded(px[f][0][i], 8, rng)
            r = ctx.push_frame_px(view, f, k * 50000)
            buf[:] = 0
            return r
        return ctx.push_frame_px_device(devs[f] + i * npx * BPP[f], f, k * 50000)

    got = _stream_words(ctx, push, order)
    ref.close()
    ctx.close()
    _assert_same_stream(want, got, "mixed formats")


@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "radtan"])
def test_batch_px_rotating_formats(B, lens):
    """6: a batch of 4 lanes (4 streams), the format rotated per step: each lane's records identical to a batch fed grey."""
    from rebvio_amd import synth
    W, H, L, steps = 640, 480, 4, 14
    streams = [synth.render_stream(W, H, 8, stream_id=l) for l in range(L)]
    cam = streams[0][1]
    pxs = [colourise(f, 11 + l) for l, (f, _) in enumerate(streams)]
    order = synth.pingpong_indices(8, steps)
    fmts = [(k + 3) % 7 for k in range(steps)]

    def run(colour):
        b = B.Batch(params_for(B, cam, **KW_C2), L)
        if lens:
            for ctx in b.lanes:
                ctx.set_undistort(cam.fm, cam.fm, cam.cx, cam.cy, EUROC_D)
        recs = [[] for _ in range(L)]
        if colour:
            devs = [{f: b.lanes[l].upload_frames(pxs[l][f][0]) for f in FMTS} for l in range(L)]
        else:  # the grey frame each step's colour frame stands for
            seq = [np.stack([pxs[l][f][1][i] for f, i in zip(fmts, order)]) for l in range(L)]
            devs = [b.lanes[l].upload_frames(seq[l]) for l in range(L)]

        def take(outs, ns):
            for l in range(L):
                if outs[l].status >= 0:
                    recs[l].append(rec(outs[l], ns[l]))

        for k, i in enumerate(order):
            f = fmts[k]
            if colour:
                take(*b.push_px_device([devs[l][f] + int(i) * W * H * BPP[f] for l in range(L)], f, k * 50000))
            else:
                take(*b.push_u8_device([devs[l] + k * W * H for l in range(L)], k * 50000))
        for outs, ns in b.flush():
            take(outs, ns)
        b.close()
        return recs

    want, got = run(False), run(True)
    for l in range(L):
        assert len(want[l]) == len(got[l]) == steps - 1, (l, len(want[l]), len(got[l]))
        for k, (a, c) in enumerate(zip(want[l], got[l])):
            assert np.array_equal(a, c), (l, k, np.flatnonzero(a != c)[:8])
        assert want[l][-1][-1] > 1000


def test_px_entries_refuse_bad_arguments(B, px_stream):
    """7: -3 and a message, before the device is touched: unknown format, odd width for YUYV / UYVY, a pitch below a row's bytes,
    a null frame. The context is usable afterwards."""
    import ctypes as C
    px, cam = px_stream
    L = B.lib()
    ctx = B.Context(params_for(B, cam, **KW_C2))
    frame = px[RGB8][0][0]
    h = C.c_void_p()
    out = B.PairOut()
    n = C.c_int()
    ptr = frame.ctypes.data_as(C.c_void_p)
    # (a real device frame behind every device pointer: a refusal that failed would still read valid memory)
    dptr = C.c_void_p(ctx.upload_frames(px[RGBA8][0][:1]))

    def refused(rc, words):
        msg = L.rebvio_hip_last_error().decode()
        assert rc == -3 and all(w in msg for w in words), (rc, msg)

    for bad in (-1, 7, 99):
        refused(L.rebvio_hip_detect_px(ctx.h, ptr, 0, bad, 0, C.byref(h)), ["unknown pixel format"])
        refused(L.rebvio_hip_detect_px_device(ctx.h, dptr, bad, 0, C.byref(h)), ["unknown pixel format"])
        refused(L.rebvio_hip_push_frame_px(ctx.h, ptr, 0, bad, 0, C.byref(out), C.byref(n)), ["unknown pixel format"])
        refused(L.rebvio_hip_push_frame_px_device(ctx.h, dptr, bad, 0, C.byref(out), C.byref(n)), ["unknown pixel format"])
        refused(L.rebvio_hip_front_end_px(ctx.h, ptr, 0, bad, np.zeros(1, np.float32).ctypes.data_as(C.POINTER(C.c_float))),
                ["unknown pixel format"])
    for fmt in FMTS:
        bpp_row = cam.width * BPP[fmt]
        refused(L.rebvio_hip_detect_px(ctx.h, ptr, bpp_row - 1, fmt, 0, C.byref(h)), ["pitch_bytes"])
        refused(L.rebvio_hip_push_frame_px(ctx.h, ptr, bpp_row - 1, fmt, 0, C.byref(out), C.byref(n)), ["pitch_bytes"])
        refused(L.rebvio_hip_detect_px(ctx.h, None, 0, fmt, 0, C.byref(h)), ["null frame"])
        refused(L.rebvio_hip_detect_px_device(ctx.h, None, fmt, 0, C.byref(h)), ["null frame"])
        refused(L.rebvio_hip_push_frame_px(ctx.h, None, 0, fmt, 0, C.byref(out), C.byref(n)), ["null frame"])
        refused(L.rebvio_hip_push_frame_px_device(ctx.h, None, fmt, 0, C.byref(out), C.byref(n)), ["null frame"])
    b = B.Batch(params_for(B, cam, **KW_C2), 2)
    bdev = [b.lanes[l].upload_frames(px[RGBA8][0][:1]) for l in range(2)]
    refused(L.rebvio_hip_batch_push_px_device(b.h, (C.c_void_p * 2)(bdev[0], None), RGB8, 0, b._out, b._n), ["null frame"])
    refused(L.rebvio_hip_batch_push_px_device(b.h, (C.c_void_p * 2)(*bdev), 8, 0, b._out, b._n), ["unknown pixel format"])
    b.close()
    # an odd width: YUYV / UYVY refused everywhere, the other formats accepted
    from rebvio_amd import synth
    g, cam_odd = synth.render_stream(131, 67, 2)
    odd = B.Context(params_for(B, cam_odd, keylines_ref=3000, keylines_max=4000))
    yuv = np.zeros((67, 131, 2), np.uint8)
    ydev = C.c_void_p(odd.upload_frames(yuv))
    for fmt in (YUYV, UYVY):
        yp = yuv.ctypes.data_as(C.c_void_p)
        refused(L.rebvio_hip_detect_px(odd.h, yp, 0, fmt, 0, C.byref(h)), ["even width"])
        refused(L.rebvio_hip_detect_px_device(odd.h, ydev, fmt, 0, C.byref(h)), ["even width"])
        refused(L.rebvio_hip_push_frame_px(odd.h, yp, 0, fmt, 0, C.byref(out), C.byref(n)), ["even width"])
        refused(L.rebvio_hip_push_frame_px_device(odd.h, ydev, fmt, 0, C.byref(out), C.byref(n)), ["even width"])
    m = odd.detect_px(np.ascontiguousarray(np.stack([g[0]] * 3, -1)), RGB8, 0)
    assert m.size() > 0
    m.release()
    odd.close()
    # nothing was queued by the refusals: the context still runs a stream
    m = ctx.detect_px(frame, RGB8, 0)
    assert m.size() > 1000
    m.release()
    ctx.close()


def _read_edge_frames(path):
    raw = np.fromfile(path, np.uint8)
    out, o = [], 0
    while o < len(raw):
        t, r, c = raw[o:o + 12].view(np.int32)
        o += 12
        nb = r * c * (1 if t == 0 else 4)
        out.append((int(t), raw[o:o + nb].copy()))
        o += nb
    return out


@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "radtan"])
def test_cpp_rebvio_takes_bgr_frames(host_lib, tmp_path, lens):
    """8: rebvio::Rebvio with IMU samples, the stream once as CV_8UC3 BGR and once as the CV_8UC1 grey frames: the odometry
    records (every float to nine digits) and the edge-image callback frames byte-identical - the undistorted fp32 frame with
    a lens model, the CV_8UC1 grey frame without."""
    from rebvio_amd import synth
    n, W, H = 22, 320, 240   # (pose integration starts after 4 + init_bias_frame_num frames, rebvio.cpp:263)
    grey0, cam = synth.render_stream(W, H, n, dist=EUROC_D if lens else None)
    px = colourise(grey0, 5)
    bgr, grey = px[BGR8]
    scene = synth.make_scene(0)
    ts, gyro, acc = synth.imu_samples(scene, n, noise_seed=1)
    rec = np.zeros(len(ts), dtype=[("ts", "<i8"), ("gyro", "<f4", 3), ("acc", "<f4", 3)])
    rec["ts"], rec["gyro"], rec["acc"] = ts, gyro, acc
    rec.tofile(tmp_path / "imu.bin")
    grey.tofile(tmp_path / "grey.u8")
    bgr.tofile(tmp_path / "bgr.u8")
    exe = str(tmp_path / "colour_frames")
    subprocess.run(["g++", "-std=c++17", "-O1"] + INC + [os.path.join(ROOT, "tests", "cpp", "test_colour_frames.cpp"), "-o", exe,
                    "-L", host_lib, "-lrebvio", "-lrebvio_hip", f"-Wl,-rpath,{host_lib}", "-pthread"], check=True)
    extra = [",".join(repr(float(np.float32(v))) for v in EUROC_D)] if lens else []

    def run(mode):
        edge = tmp_path / f"edge_{mode}.bin"
        r = subprocess.run([exe, mode, str(tmp_path / f"{mode}.u8"), str(W), str(H), str(n), repr(cam.fm), repr(cam.cx), repr(cam.cy),
                            str(tmp_path / "imu.bin"), str(edge)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (mode, r.stdout[-1000:], r.stderr[-2000:])
        return r.stdout, _read_edge_frames(edge)

    (odo_g, edge_g), (odo_c, edge_c) = run("grey"), run("bgr")
    lines = odo_g.strip().splitlines()
    assert len(lines) == n - 1 and odo_c == odo_g
    assert abs(float(lines[-1].split()[4])) + abs(float(lines[-1].split()[6])) > 0   # the pose moved
    assert len(edge_g) == len(edge_c) == n
    for k, ((tg, bg), (tc, bc)) in enumerate(zip(edge_g, edge_c)):
        assert tg == tc == (5 if lens else 0), (k, tg, tc)
        assert np.array_equal(bg, bc), k
    if not lens:
        assert np.array_equal(edge_c[0][1].reshape(H, W), grey[0])


def test_replay_colour_flag_writes_the_same_odometry(host_lib, tmp_path):
    """9: rebvio_replay on an RGB ASL folder: --colour (RGB frames to the device as they are, converted there) writes the same
    odometry file, byte for byte, as the default (luma on the host while reading)."""
    from pngutil import write_asl
    from rebvio_amd import synth
    n, W, H = 12, 320, 240
    grey0, cam = synth.render_stream(W, H, n)
    rgb = colourise(grey0, 9)[RGB8][0]
    scene = synth.make_scene(0)
    its, gyro, acc = synth.imu_samples(scene, n, noise_seed=1)
    ts = np.arange(n) * 50000 + 1000000
    write_asl(str(tmp_path / "mav0"), rgb, ts, its + 1000000, gyro, acc, filters=(1, 4))
    exe = os.path.join(host_lib, "rebvio_replay")
    common = ["--asl", str(tmp_path / "mav0"), "--camera", repr(cam.fm), repr(cam.cx), repr(cam.cy), "--keylines", "3000", "4000",
              "--min-matches", "50"]
    r1 = subprocess.run([exe] + common + ["--out", str(tmp_path / "grey.txt")], capture_output=True, text=True, timeout=300)
    r2 = subprocess.run([exe] + common + ["--colour", "--out", str(tmp_path / "colour.txt")], capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr[-1500:], r2.stderr[-1500:])
    a, b = (tmp_path / "grey.txt").read_bytes(), (tmp_path / "colour.txt").read_bytes()
    assert len(a.splitlines()) == n - 1 and a == b
