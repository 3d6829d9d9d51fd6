"""The depth prior from a registered depth image on the GPU (rebvio_hip_map_fuse_depth_image*, k_depth_prior).

Maps are crafted through rebvio_hip_map_upload (a context of keylines_max = n detects exactly n keylines on a checkerboard frame;
the upload then replaces them) and every word the device leaves - rho, sigma_rho, the outcome words, the counts - is compared with
the host hook (rebvio_hip_test_depth_prior_host, the same statements in index order), which tests/test_depth_prior.py holds against
the numpy restatement of the header. Every comparison is equality."""
import ctypes as C
import functools

import numpy as np
import pytest

import depth_prior_ref as R
from conftest import params_for
from support import B, refusal_scene  # noqa: F401
from support import DEAD_MAP, assert_refused
from support import (F32, KW_TRACK, assert_keylines_equal, noise_frames, oracle_fusion, rec, same_records, vision_only_fusion,
                     words)

pytestmark = pytest.mark.gpu

NAN = F32(np.nan)
MID_FIELDS = ("Vg", "P_Vg", "F", "sigma_rho_min", "Xv", "W_Xv", "Xgv")


def checker(rows, cols):
    """6-pixel checkerboard: 299 keylines at 32x32 with the threshold below, enough for maps of 257"""
    y, x = np.mgrid[0:rows, 0:cols]
    return ((((x // 6) + (y // 6)) % 2) * 200 + 20).astype(np.uint8)


def sized_ctx(B, n, rows=32, cols=32):
    from rebvio_amd import synth
    cam = synth.Camera.for_size(cols, rows)
    return B.Context(params_for(B, cam, keylines_ref=max(1, n - 1), keylines_max=max(1, n), threshold=0.001, gain=0.0,
                                global_min_matches_threshold=1))


def sized_map(ctx, n, ts=0):
    rows, cols = ctx.rows, ctx.cols
    m = ctx.detect_u8(checker(rows, cols) if n else np.full((rows, cols), 128, np.uint8), ts)
    assert m.size() == n, (m.size(), n)
    return m


def random_keylines(B, n, rows, cols, seed):
    rng = np.random.default_rng(seed)
    kl = np.zeros(n, B.KEYLINE_DTYPE)
    kl["pos"] = rng.uniform(-3, max(rows, cols) + 3, (n, 2)).astype(F32)
    kl["pos_img"] = rng.normal(0, 50, (n, 2)).astype(F32)   # (not what the taps use)
    kl["gradient"] = rng.normal(0, 5, (n, 2)).astype(F32)
    kl["gradient_norm"] = np.sqrt((kl["gradient"].astype(np.float64) ** 2).sum(1)).astype(F32)
    kl["rho"] = rng.uniform(0.001, 3, n).astype(F32)
    kl["sigma_rho"] = rng.uniform(0, 2, n).astype(F32)
    kl["matches"] = rng.integers(0, 9, n)
    kl["id_prev"] = kl["id_next"] = kl["match_id"] = kl["match_id_forward"] = kl["match_id_keyframe"] = -1
    return kl


def random_image(rows, cols, fmt, seed, pad=0):
    rng = np.random.default_rng(seed)
    if fmt == 1:
        img = rng.uniform(0, 25, (rows, cols + pad)).astype(F32)
        img[rng.uniform(size=img.shape) < 0.05] = NAN
    else:
        img = rng.integers(0, 25000, (rows, cols + pad)).astype(np.uint16)
        img[rng.uniform(size=img.shape) < 0.1] = 0
    return img[:, :cols]


def check(B, m, kl, img, fmt=None, opts=None, entry="host", what=""):
    """upload kl, fuse img through `entry`, compare everything with the hook; -> the counts tuple"""
    ctx = m.ctx
    m.upload(kl)
    back = m.keylines()                                  # what the map holds (`id` is not kept on the device)
    for f in ("pos", "gradient", "gradient_norm", "rho", "sigma_rho", "matches"):
        assert back[f].tobytes() == kl[f].tobytes(), f
    want_c, want_kl, want_oc = B.depth_prior_host(ctx.rows, ctx.cols, back, img, fmt, opts)
    if entry == "host":
        got_c, got_oc = m.fuse_depth_image(img, fmt, opts, want_outcome=True)
    else:
        keep, _, pitch, f = B._depth_image(img, fmt, ctx.rows, ctx.cols)
        padded = np.ones((ctx.rows, pitch // keep.itemsize), keep.dtype)  # the same pitch on the device, valid depths in the padding
        padded[:, :ctx.cols] = keep
        dev = ctx.upload_bytes(padded)
        if entry == "device":
            got_c, got_oc = m.fuse_depth_image(dev, f, opts, device=True, pitch=pitch, want_outcome=True)
        else:
            assert m.fuse_depth_image(dev, f, opts, queued=True, pitch=pitch) is None
            got_c, got_oc = ctx.depth_prior_last_counts(), None
    assert got_c.as_tuple() == want_c.as_tuple(), (what, entry, got_c.as_tuple(), want_c.as_tuple())
    if got_oc is not None:
        assert np.array_equal(got_oc, want_oc), (what, entry, np.flatnonzero(got_oc != want_oc)[:8])
    assert_keylines_equal(want_kl, m.keylines(), what=f"{what} ({entry})")
    return got_c.as_tuple()


def padded_source(img, pad):
    """the same image as a column slice of a wider array: pitch > width"""
    wide = np.zeros((img.shape[0], img.shape[1] + pad), img.dtype)
    wide[:, :img.shape[1]] = img
    wide[:, img.shape[1]:] = 1 if img.dtype == np.uint16 else 1.0  # valid depths in the padding: a tap that strays there shows
    return wide[:, :img.shape[1]]


# ---- sizes, formats, entries ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_sizes_around_the_workgroup(B, n):
    ctx = sized_ctx(B, n)
    m = sized_map(ctx, n)
    for fmt in (0, 1):
        c = check(B, m, random_keylines(B, n, 32, 32, 10 + n + fmt), random_image(32, 32, fmt, n + fmt), fmt, what=f"n={n} fmt={fmt}")
        assert c[0] == n and (n < 255 or (c[2] > 20 and c[3] > 5)), c
    ctx.close()


@pytest.mark.parametrize("fmt", [0, 1])
def test_pitch_above_width_on_37x33_and_the_three_entries(B, fmt):
    ctx = sized_ctx(B, 257, rows=33, cols=37)
    m = sized_map(ctx, 257)
    kl = random_keylines(B, 257, 33, 37, 77 + fmt)
    img = padded_source(random_image(33, 37, fmt, 5 + fmt), 5)
    assert img.strides[0] == (37 + 5) * img.itemsize
    counts = {e: check(B, m, kl, img, fmt, entry=e, what=f"37x33 fmt={fmt}") for e in ("host", "device", "queued")}
    assert counts["host"] == counts["device"] == counts["queued"] and counts["host"][2] > 20, counts
    # ... and with options off their defaults
    opts = B.default_depth_prior_opts(tap_px=3.5, jump_rel=0.3, q_abs=0.5, gate_sigma=1.5, unit=0.0007)
    for e in ("host", "device", "queued"):
        check(B, m, kl, img, fmt, opts, entry=e, what="options")
    ctx.close()


def test_last_counts_follow_the_most_recent_fusion(B):
    ctx = sized_ctx(B, 257)
    assert ctx.depth_prior_last_counts().as_tuple() == (0, 0, 0, 0, 0, 0)   # nothing yet
    m = sized_map(ctx, 257)
    kl = random_keylines(B, 257, 32, 32, 3)
    a = check(B, m, kl, random_image(32, 32, 1, 1), 1, entry="queued", what="first")
    b = check(B, m, kl, np.full((32, 32), 0.01, F32), 1, entry="queued", what="second: no valid depth")
    assert a[1] > 0 and b == (257, 0, 0, 0, 0, 0)
    assert ctx.depth_prior_last_counts().as_tuple() == b                    # read twice
    c = check(B, m, kl, random_image(32, 32, 0, 2), 0, entry="host", what="third")
    assert ctx.depth_prior_last_counts().as_tuple() == c
    ctx.close()


# ---- planted cases (tests/test_depth_prior.py works their outcomes out by hand) ----------------------------------------------------
def test_planted_cases(B):
    rows, cols = 33, 37
    ctx = sized_ctx(B, 40, rows=rows, cols=cols)
    m = sized_map(ctx, 40)
    kl = np.zeros(40, B.KEYLINE_DTYPE)
    kl["rho"], kl["sigma_rho"], kl["gradient"], kl["gradient_norm"] = 1.0, 20.0, (1.0, 0.0), 1.0
    kl["pos"] = (10.0, 10.0)
    img = np.full((rows, cols), 2.0, F32)
    img[:, 0] = img[:, cols - 1] = img[0, :] = img[rows - 1, :] = 1.0
    P, G = kl["pos"], kl["gradient"]
    # taps on each border and just outside
    P[0], G[0] = (2.0, 10.0), (-1.0, 0.0)
    P[1], G[1] = (cols - 3.0, 10.0), (1.0, 0.0)
    P[2], G[2] = (10.0, 2.0), (0.0, -1.0)
    P[3], G[3] = (10.0, rows - 3.0), (0.0, 1.0)
    P[4], G[4] = (1.25, 10.0), (-1.0, 0.0)
    P[5], G[5] = (cols - 2.5, 10.0), (1.0, 0.0)
    P[6], G[6] = (10.0, 1.25), (0.0, -1.0)
    P[7], G[7] = (10.0, rows - 2.5), (0.0, 1.0)
    P[8], G[8] = (1.5, 10.0), (-1.0, 0.0)
    P[9] = (-1.0, 10.0)
    # no usable direction: the centre tap alone (the side taps would see the 1.0 planted at (12, 20) and (8, 20))
    img[20, 12] = img[20, 8] = 1.0
    P[10:15] = (10.0, 20.0)
    kl["gradient_norm"][10:14] = (1.0, 0.0, NAN, -1.0)
    G[14] = (np.inf, 0.0)
    # bad positions
    P[15], P[16], P[17], P[18] = (NAN, 5.0), (5.0, np.inf), (-np.inf, NAN), (1e30, 5.0)
    # all taps invalid
    img[25:28, 20:27] = 0.05
    P[19] = (23.0, 26.0)
    img[25:28, 28:35] = NAN
    P[20] = (31.0, 26.0)
    # a jump exactly at jump_rel = 0.5 and one ulp over
    img[14, 22] = 3.0
    P[21] = (20.0, 14.0)
    img[16, 22] = np.nextafter(F32(3.0), F32(4.0))
    P[22] = (20.0, 16.0)
    # sigma_rho 0: agreeing, disagreeing; a keyline far from the sensor's depth but wide open
    P[23:26] = (16.0, 5.0)
    kl["rho"][23:26], kl["sigma_rho"][23:26] = (0.5, 0.6, 19.0), (0.0, 0.0, 20.0)
    opts = B.default_depth_prior_opts(jump_rel=0.5)
    want = [17, 17, 17, 17, 1, 1, 1, 1, 17, 1, 17, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 17, 1, 2, 1] + [1] * 14
    c, _, oc = B.depth_prior_host(rows, cols, kl, img, 1, opts)
    assert list(oc) == want, list(oc)
    for e in ("host", "device", "queued"):
        check(B, m, kl, img, 1, opts, entry=e, what="planted")
    # u16 value 0 (centre alone, then everywhere), the innovation exactly at the gate, both clamps
    img16 = np.full((rows, cols), 2000, np.uint16)
    img16[10, 10] = 0
    kl2 = kl.copy()
    kl2["pos"], kl2["gradient"], kl2["gradient_norm"] = (10.0, 10.0), (1.0, 0.0), 1.0
    c = check(B, m, kl2, img16, 0, what="u16 zero at the centre")
    assert c[1] == 40
    assert check(B, m, kl2, np.zeros((rows, cols), np.uint16), 0, what="u16 all zero") == (40, 0, 0, 0, 0, 0)
    kl2["sigma_rho"] = 0.0
    kl2["rho"] = 0.25
    kl2["rho"][:2] = (1.0, np.nextafter(F32(1.0), F32(2.0)))
    gate = B.default_depth_prior_opts(sigma_z0=0.0, sigma_z2=0.25, gate_sigma=2.0)
    c = check(B, m, kl2, np.full((rows, cols), 2.0, F32), 1, gate, what="at the gate")
    assert c == (40, 40, 39, 1, 0, 0), c
    kl2["rho"], kl2["sigma_rho"] = 1.0, 20.0
    clamp = np.full((rows, cols), 0.04, F32)
    clamp[:, 18:] = 2000.0
    kl2["pos"][:20] = (5.0, 5.0)
    kl2["pos"][20:] = (30.0, 5.0)
    c = check(B, m, kl2, clamp, 1, B.default_depth_prior_opts(z_min=0.01, z_max=5000.0, tap_px=0.0), what="both clamps")
    assert c == (40, 40, 40, 0, 0, 40), c
    back = m.keylines()
    assert (back["rho"][:20] == F32(20.0)).all() and (back["rho"][20:] == F32(1e-3)).all()
    ctx.close()


# ---- re-use, the envelope ----------------------------------------------------------------------------------------------------------
def test_sizes_257_3_0_257_in_one_context(B):
    ctx = sized_ctx(B, 257)
    m_a = sized_map(ctx, 257, 0)
    ctx.set_detection_mask(((m_a.mask() >= 0) & (m_a.mask() < 3)).astype(np.uint8))
    m_3 = ctx.detect_u8(checker(32, 32), 50000)
    ctx.set_detection_mask(None)
    m_0 = sized_map(ctx, 0, 100000)
    m_b = sized_map(ctx, 257, 150000)
    assert (m_3.size(), m_0.size()) == (3, 0)
    img = random_image(32, 32, 1, 9)
    for what, m, seed in (("257", m_a, 1), ("3", m_3, 2), ("0", m_0, 3), ("257 again", m_b, 4), ("3 again", m_3, 5)):
        for e in ("host", "queued"):
            c = check(B, m, random_keylines(B, m.size(), 32, 32, seed), img, 1, entry=e, what=what)
            assert c[0] == m.size()
    ctx.close()


def test_the_full_envelope_of_65536_keylines(B):
    frame = noise_frames(896, 640, 1, 3)[0]      # a noise frame of this size holds more candidates than the envelope
    ctx = B.Context(B.default_params(640, 896, fm=500.0, cx=447.5, cy=319.5, keylines_ref=60000, keylines_max=65536))
    m = ctx.detect_u8(frame, 0)
    assert m.size() == 65536
    kl = m.keylines()
    rng = np.random.default_rng(4)
    kl["rho"] = rng.uniform(0.05, 2, len(kl)).astype(F32)
    kl["sigma_rho"] = rng.uniform(0, 1, len(kl)).astype(F32)
    img = rng.integers(0, 12000, (640, 896)).astype(np.uint16)
    c = check(B, m, kl, img, 0, what="65536 keylines")
    assert c[0] == 65536 and c[1] > 60000 and c[2] > 1000 and c[3] > 1000, c
    ctx.close()


# ---- refusals, resources, launches --------------------------------------------------------------------------------------------------
def test_refusals_minus_7_minus_10_and_minus_3(B, small_stream):
    frames, cam = small_stream
    ctx = B.Context(params_for(B, cam, **KW_TRACK))
    maps = [ctx.detect_u8(frames[i], i * 50000) for i in range(4)]
    depth = np.full((cam.height, cam.width), 2.0, F32)
    dev = ctx.upload_bytes(depth)
    c, s = F32(np.cos(0.01)), F32(np.sin(0.01))
    Rn = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], F32)
    assert maps[0].fuse_depth_image(depth).fused > 0                    # a stream's first map, right after detection
    mid = ctx.track_pair_begin(maps[0], maps[1])
    ctx.track_pair_finish_async(maps[0], maps[1], *vision_only_fusion(mid), R_prior_next=Rn)
    ctx.track_pair_result()
    for call in (lambda: maps[1].fuse_depth_image(depth), lambda: maps[1].fuse_depth_image(dev, B.DEPTH_F32, device=True),
                 lambda: maps[1].fuse_depth_image(dev, B.DEPTH_F32, queued=True)):
        with pytest.raises(B.HipError) as e:
            call()
        assert "error -7:" in str(e.value) and "R_prior_next" in str(e.value), str(e.value)   # promised: rotated for the next pair
    with pytest.raises(B.HipError) as e:
        maps[0].fuse_depth_image(depth)                                                       # has served as an old map
    assert "error -7:" in str(e.value) and "old map" in str(e.value), str(e.value)
    mid = ctx.track_pair_begin(maps[1], maps[2], R_prior=Rn)
    ctx.track_pair_finish_async(maps[1], maps[2], *vision_only_fusion(mid))
    ctx.track_pair_result()
    with pytest.raises(B.HipError) as e:
        maps[1].fuse_depth_image(depth)                                   # the promise is consumed, but now it has served as old
    assert "error -7:" in str(e.value) and "old map" in str(e.value)
    assert maps[2].fuse_depth_image(depth).fused > 0                      # the new map of the last pair is where the image belongs
    # -3 with a live map: options, format, pitch; a map of another context through the queued entry
    L = B.lib()
    cnt = B.DepthPriorCounts()
    bad = B.default_depth_prior_opts(z_min=0.0)
    assert L.rebvio_hip_map_fuse_depth_image(maps[3].h, depth.ctypes.data, 0, 1, bad, C.byref(cnt), None) == -3
    assert L.rebvio_hip_map_fuse_depth_image(maps[3].h, depth.ctypes.data, 0, 7, None, C.byref(cnt), None) == -3
    assert L.rebvio_hip_map_fuse_depth_image(maps[3].h, depth.ctypes.data, cam.width * 4 - 4, 1, None, C.byref(cnt), None) == -3
    assert L.rebvio_hip_map_fuse_depth_image(maps[3].h, None, 0, 1, None, C.byref(cnt), None) == -3
    assert L.rebvio_hip_map_fuse_depth_image_device(maps[3].h, C.c_void_p(dev), 0, 1, None, None, None) == -3
    other = B.Context(params_for(B, cam, **KW_TRACK))
    assert L.rebvio_hip_map_fuse_depth_image_async(other.h, maps[3].h, C.c_void_p(dev), 0, 1, None) == -3
    other.close()
    ctx.close()
    assert L.rebvio_hip_map_fuse_depth_image(maps[3].h, depth.ctypes.data, 0, 1, None, C.byref(cnt), None) == -10
    assert "destroyed" in L.rebvio_hip_last_error().decode()
    assert L.rebvio_hip_map_fuse_depth_image_device(maps[3].h, C.c_void_p(dev), 0, 1, None, C.byref(cnt), None) == -10
    for m in maps:
        m.release()


def test_one_launch_per_call_and_one_allocation(B):
    """k_depth_prior once per call whatever the map holds; the first call of a device-image entry gives the context one live
    resource (the counts and outcome words), the first host-image call its pinned staging frame, and no call after that anything;
    a refused call allocates nothing; nothing is left after destroy"""
    live = B.test_live_resources()
    ctx = sized_ctx(B, 257)
    m, m0 = sized_map(ctx, 257, 0), sized_map(ctx, 0, 50000)
    m.upload(random_keylines(B, 257, 32, 32, 1))
    m.keylines()
    m0.keylines()
    img = random_image(32, 32, 1, 1)
    dev = ctx.upload_bytes(np.ascontiguousarray(img))
    base = B.test_live_resources()
    with pytest.raises(B.HipError):
        m.fuse_depth_image(dev, B.DEPTH_F32, B.default_depth_prior_opts(unit=0.0), device=True)
    assert B.test_live_resources() == base
    ctx.profile(True)
    for k, (mm, kw) in enumerate(((m, dict(device=True)), (m0, dict(device=True)), (m, dict(queued=True)), (m, dict(device=True)))):
        ctx.profile_reset()
        mm.fuse_depth_image(dev, B.DEPTH_F32, **kw)
        ctx.depth_prior_last_counts()
        launches = {name: calls for name, (_, calls) in ctx.profile_read().items() if calls}
        assert launches == {"k_depth_prior": 1}, (k, launches)
        assert B.test_live_resources() == base + 1, k
    for k in range(3):
        ctx.profile_reset()
        (m if k != 1 else m0).fuse_depth_image(img)
        launches = {name: calls for name, (_, calls) in ctx.profile_read().items() if calls}
        assert launches == {"k_depth_prior": 1}, (k, launches)
        assert B.test_live_resources() == base + 2, k
    ctx.profile(False)
    ctx.close()
    m.release()
    m0.release()
    assert B.test_live_resources() == live


# ---- with the tracker -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stream_depth(width, height, n):
    from rebvio_amd import synth
    return synth.render_stream_depth(width, height, n)


@pytest.fixture(scope="module")
def oracle_runs(orc_mod, small_stream):
    """the 192x144 stream's first 10 frames through the oracle, with the restatement fusing every frame's depth and without"""
    frames, cam = small_stream
    depth = stream_depth(cam.width, cam.height, 10)
    p = params_for(orc_mod, cam, **KW_TRACK)
    return R.oracle_stream(orc_mod, p, frames[:10], depth, True), R.oracle_stream(orc_mod, p, frames[:10], depth, False)


def test_pipeline_through_track_pair_equals_oracle_plus_restatement(B, small_stream, oracle_runs):
    """fusion between the pairs of rebvio_hip_track_pair: every word of every pair record, the counts of every fusion and every
    keyline field of the newest map equal the oracle-plus-restatement run; host and device entries in turn"""
    frames, cam = small_stream
    depth = stream_depth(cam.width, cam.height, 10)
    want = oracle_runs[0]
    ctx = B.Context(params_for(B, cam, **KW_TRACK))
    dev = ctx.upload_bytes(depth)
    maps = [ctx.detect_u8(frames[k], k * 50000) for k in range(10)]
    for k in range(10):
        if k:
            pg = ctx.track_pair(maps[k - 1], maps[k])
            wo, wg = rec(want["records"][k - 1], want["sizes"][k - 1]), rec(pg, maps[k].size())
            assert np.array_equal(wo, wg), (k, np.flatnonzero(wo != wg)[:8])
        if k % 2:
            c = maps[k].fuse_depth_image(depth[k])
        else:
            c = maps[k].fuse_depth_image(dev + k * depth[k].nbytes, B.DEPTH_F32, device=True)
        assert c.as_tuple() == R.counts_tuple(want["counts"][k]), (k, c.as_tuple(), want["counts"][k])
    assert_keylines_equal(want["keylines"], maps[9].keylines(), what="newest map after 9 pairs with depth")
    assert all(r.status == 0 for r in want["records"])
    with pytest.raises(B.HipError) as e:
        maps[8].fuse_depth_image(depth[8])                                # rebvio_hip_track_pair marks its old map
    assert "error -7:" in str(e.value) and "old map" in str(e.value), str(e.value)
    ctx.close()


def test_pipeline_through_the_split_api_with_the_queued_entry(orc_mod, B, small_stream, oracle_runs):
    """the same through rebvio_hip_track_pair_begin / _finish_async, the fusion queued between _finish_async(k) and _begin(k + 1)
    and nothing waited for in between (the order rebvio::Rebvio uses); handed the oracle's own fusion results the halves reproduce
    the oracle-plus-restatement run: the first half's record, the second half's counters, the fusions' counts, the newest map"""
    frames, cam = small_stream
    depth = stream_depth(cam.width, cam.height, 10)
    want = oracle_runs[0]
    ctx = B.Context(params_for(B, cam, **KW_TRACK))
    dev = ctx.upload_bytes(depth)
    maps = [ctx.detect_u8(frames[k], k * 50000) for k in range(10)]
    maps[0].fuse_depth_image(dev, B.DEPTH_F32, queued=True)
    for k in range(1, 10):
        po = want["records"][k - 1]
        mid = ctx.track_pair_begin(maps[k - 1], maps[k])
        if k > 1:
            assert ctx.track_pair_result() == (pp.klm_num, pp.kf_matches, pp.reg_num, pp.status), k
        for f in MID_FIELDS:
            assert np.array_equal(words(getattr(mid, f)), words(getattr(po, f))), (k, f)
        ctx.track_pair_finish_async(maps[k - 1], maps[k], *oracle_fusion(orc_mod, po))
        maps[k].fuse_depth_image(dev + k * depth[k].nbytes, B.DEPTH_F32, queued=True)
        if k in (1, 5, 9):
            assert ctx.depth_prior_last_counts().as_tuple() == R.counts_tuple(want["counts"][k]), k
        pp = po
    assert ctx.track_pair_result() == (pp.klm_num, pp.kf_matches, pp.reg_num, pp.status)
    assert_keylines_equal(want["keylines"], maps[9].keylines(), what="newest map, split API with queued fusions")
    ctx.close()


def test_a_stream_without_a_depth_call_is_unchanged(B, small_stream, oracle_runs):
    """no depth call: the records are the oracle's word for word (the old-map flag costs nothing)"""
    frames, cam = small_stream
    want = oracle_runs[1]
    ctx = B.Context(params_for(B, cam, **KW_TRACK))
    maps = [ctx.detect_u8(frames[k], k * 50000) for k in range(10)]
    got = [rec(ctx.track_pair(maps[k - 1], maps[k]), maps[k].size()) for k in range(1, 10)]
    same_records([rec(r, n) for r, n in zip(want["records"], want["sizes"])], got, "no depth")
    assert_keylines_equal(want["keylines"], maps[9].keylines(), what="newest map without depth")
    ctx.close()


# ---- the refusal table: every shared refusal with its code and whole text; which one wins when several apply ------

IMG = "map_fuse_depth_image"
_depth = lambda s: np.full((s.ctx.rows, s.ctx.cols), 2.0, np.float32)
_do = lambda s, **kw: s.B.default_depth_prior_opts(**kw)
_queued = lambda s, m: s.B.lib().rebvio_hip_map_fuse_depth_image_async(s.other.h, m.h, C.c_void_p(256), 0, 1, None)
REFUSED = {
    "queued: map of another context": (lambda s: _queued(s, s.m), -3, "map_fuse_depth_image_async: map of another context"),
    "queued: wins: a destroyed map over another context": (lambda s: _queued(s, s.dm), -10, DEAD_MAP),
    "destroyed map": (lambda s: s.dm.fuse_depth_image(_depth(s)), -10, DEAD_MAP),
    "gate_sigma": (lambda s: s.m.fuse_depth_image(_depth(s), opts=_do(s, gate_sigma=0.0)), -3, f"{IMG}: gate_sigma must be > 0"),
    "q_abs": (lambda s: s.m.fuse_depth_image(_depth(s), opts=_do(s, q_abs=-1.0)), -3, f"{IMG}: q_abs must be >= 0"),
    "wins: a destroyed map over an option": (lambda s: s.dm.fuse_depth_image(_depth(s), opts=_do(s, q_abs=-1.0)), -10, DEAD_MAP),
    "wins: the sigmas over gate_sigma": (lambda s: s.m.fuse_depth_image(_depth(s), opts=_do(s, sigma_z0=0.0, sigma_z2=0.0, gate_sigma=0.0)), -3,
                                         f"{IMG}: sigma_z0 + sigma_z2 must be > 0"),
    "wins: gate_sigma over q_abs": (lambda s: s.m.fuse_depth_image(_depth(s), opts=_do(s, gate_sigma=0.0, q_abs=-1.0)), -3,
                                    f"{IMG}: gate_sigma must be > 0"),
    "wins: q_abs over unit": (lambda s: s.m.fuse_depth_image(_depth(s), opts=_do(s, q_abs=-1.0, unit=0.0)), -3, f"{IMG}: q_abs must be >= 0"),
}

@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusal_table(refusal_scene, case):
    """every refusal of the table with its return code and its whole rebvio_hip_last_error text; nothing is allocated"""
    assert_refused(refusal_scene, *REFUSED[case])
