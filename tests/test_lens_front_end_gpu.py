"""The lens front end on the device (k_front_end_u8, k_front_end_px, their batched forms) off the one centred fx == fy camera the
other files use: the cameras and planted pixels of tests/lens_cases.py. Every comparison is bit equality.

The device map is read back through the public entry: front_end_u8 of the two ramp frames times 32 / 3 is the map word wherever
all four taps are inside (lens_cases.ramp_frames), so no test hook downloads it. It is held to rint of the longdouble statement
(lens_cases.direct_map); tests/test_lens_front_end.py asserts on the CPU that every case used here keeps 1e-6 of a 1/32 px unit
away from a rounding tie and holds the oracle and hm::undistort_fixed_map to the same statement."""
import ctypes as C

import numpy as np
import pytest

import lens_cases as lc
from conftest import params_for
from support import B  # noqa: F401
from support import (KW_C2, KW_TRACK, NAMES, RGB8, TS, UYVY, assert_keylines_equal, assert_refused, bits_equal, colourise, noise_frames,
                     rec, record_words, same_records)

pytestmark = pytest.mark.gpu

KW_SMALL = dict(keylines_ref=600, keylines_max=800)
COMMON = (188, 120)          # every small camera at one even-width size: a 3-byte format and UYVY through one context


def context(B, cols, rows, **kw):
    """a context of cols x rows; its own fm, cx, cy play no part in the front end"""
    return B.Context(B.default_params(rows, cols, fm=0.8 * cols, cx=cols / 2, cy=rows / 2, **dict(KW_SMALL, **kw)))


def oracle(orc_mod, cols, rows, **kw):
    return orc_mod.Oracle(orc_mod.default_params(rows, cols, fm=0.8 * cols, cx=cols / 2, cy=rows / 2, **dict(KW_SMALL, **kw)))


def set_model(ctx, case):
    ctx.set_undistort(*lc.K4(case), lc.D5(case))


def padded(frame, pad, rng):
    """frame [H, W(, bpp)] as a view into rows of pitch W * bpp + pad whose padding holds garbage"""
    H, W = frame.shape[:2]
    bpp = 1 if frame.ndim == 2 else frame.shape[2]
    buf = rng.integers(0, 256, (H, W * bpp + pad), dtype=np.uint8)
    buf[:, :W * bpp] = frame.reshape(H, W * bpp)
    return np.lib.stride_tricks.as_strided(buf, (H, W, bpp), (buf.strides[0], bpp, 1))


# ---- the device map against the direct statement ---------------------------------------------------------------------------
@pytest.mark.parametrize("size", lc.MAP_SIZES, ids=[f"{c}x{r}" for c, r in lc.MAP_SIZES])
def test_device_map_equals_the_direct_statement(B, size):
    """Every small camera at 37x33 (1221 pixels: a partial last workgroup), 131x67, 188x120 and 255x255, one context per size and
    the model changed on it from camera to camera: the map decoded from the ramp frames equals rint(direct_map) word for word
    where all four taps are inside, and both ramp images equal the zero-border formula of those words on every pixel."""
    cols, rows = size
    ctx = context(B, cols, rows)
    ramps = lc.ramp_frames(cols, rows)
    for name in lc.SMALL:
        case = lc.at_size(lc.CAMERAS[name], cols, rows)
        iu, iv = lc.map_words(case)
        inside = lc.inside(iu, iv, cols, rows)
        assert inside.sum() > cols * rows // 4, name
        set_model(ctx, case)
        for ramp, words, axis in zip(ramps, (iu, iv), "uv"):
            out = ctx.front_end_u8(ramp)
            got, exact = lc.decode_ramp(out)
            assert exact[inside].all() and np.array_equal(got[inside], words[inside]), (name, axis, int((got != words)[inside].sum()))
            assert bits_equal(out, lc.remap(iu, iv, ramp)), (name, axis)
    ctx.close()


# ---- device against oracle on random frames, grey and colour --------------------------------------------------------------
def _random_frame_cases():
    cases = {name: lc.at_size(lc.CAMERAS[name], *COMMON) for name in lc.SMALL}
    cases.update({f"planted {name}": lc.planted(name)[0] for name in lc.PLANTS})
    return cases


@pytest.mark.parametrize("group", ["table", "planted"])
def test_random_frames_equal_the_oracle_grey_and_colour(orc_mod, B, group):
    """front_end_u8, and front_end_px of RGB8 and UYVY frames, dense and with a padded pitch, for every small camera (at 188x120)
    and every planted camera (96x64): bit-equal to the oracle's front end of the grey frame; a planted pixel reads the value
    written out by hand from its words (the border past a short and past an int)."""
    cases = {n: c for n, c in _random_frame_cases().items() if n.startswith("planted") == (group == "planted")}
    cols, rows = next(iter(cases.values()))[:2]
    ctx, orc = context(B, cols, rows), oracle(orc_mod, cols, rows)
    px = colourise(np.maximum(noise_frames(cols, rows, 2, 11), 1), 12)
    rng = np.random.default_rng(13)
    for name, case in cases.items():
        assert case[:2] == (cols, rows)
        set_model(ctx, case)
        for i in range(2):
            grey = px[RGB8][1][i] if i else px[UYVY][1][i]      # the grey frame of a colour frame, and the Y plane
            want = orc.front_end_u8(grey, *lc.K4(case), lc.D5(case))
            assert bits_equal(want, ctx.front_end_u8(grey)), (name, i)
            if group == "planted":
                row, col = lc.planted(name[len("planted "):])[1]
                assert want[row, col] == lc.planted_value(name[len("planted "):], grey), name
        for fmt in (RGB8, UYVY):
            frames, grey = px[fmt]
            want = orc.front_end_u8(grey[0], *lc.K4(case), lc.D5(case))
            assert bits_equal(want, ctx.front_end_px(frames[0], fmt)), (name, NAMES[fmt])
            assert bits_equal(want, ctx.front_end_px(padded(frames[0], 20, rng), fmt)), (name, NAMES[fmt], "padded")
    ctx.close()


# ---- stripes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", lc.STRIPE_WIDTHS)
def test_stripes_device_oracle_and_direct_statement_agree(orc_mod, B, cols):
    """Widths 1365, 1366 and 4096: cv::undistort builds its map in stripes of 3, 2 and 1 rows with the principal point shifted
    per stripe. 35 rows - a context takes 32 at least, and 35 is the fewest from there that leave the last stripe of 3 and of 2
    rows ragged - with cy off the centre and fx != fy. A ramp cannot decode a map this wide; the images of the
    (7 col + 13 row) & 255 frame are compared, device against oracle against the formula of rint(direct_map)."""
    case = lc.stripe_case(cols)
    rows = case[1]
    assert rows % 3 and rows % 2 and 4096 // cols == {1365: 3, 1366: 2, 4096: 1}[cols]
    frame = lc.weave_frame(cols, rows)
    ctx = context(B, cols, rows, keylines_ref=3000, keylines_max=4000)
    set_model(ctx, case)
    got = ctx.front_end_u8(frame)
    ctx.close()
    want = oracle(orc_mod, cols, rows).front_end_u8(frame, *lc.K4(case), lc.D5(case))
    assert bits_equal(want, got), "device against oracle"
    assert bits_equal(lc.remap(*lc.map_words(case), frame), got), "device against the direct statement"


# ---- the full EuRoC camera ----------------------------------------------------------------------------------------------
def test_the_full_euroc_camera(orc_mod, B):
    """752x480 with the EuRoC intrinsics (fx != fy, principal point off the centre), 3 frames of a stream seen through that lens:
    front_end_u8 bit-equal to the oracle's, and detect_u8_host equal to the oracle's detection of the oracle's front end, keyline
    for keyline, the threshold included."""
    from rebvio_amd import synth
    case = lc.CAMERAS["euroc-full"]
    cols, rows = case[:2]
    frames, _ = synth.render_stream(cols, rows, 3, dist=list(case[6]))
    ctx, orc = context(B, cols, rows, **KW_C2), oracle(orc_mod, cols, rows, **KW_C2)
    set_model(ctx, case)
    for i in range(3):
        und = orc.front_end_u8(frames[i], *lc.K4(case), lc.D5(case))
        assert bits_equal(und, ctx.front_end_u8(frames[i])), i
        om, gm = orc.detect(und, i * TS), ctx.detect_u8_host(frames[i], i * TS)
        assert_keylines_equal(om.keylines(), gm.keylines(), what=f"euroc-full frame {i}")
        assert om.threshold == gm.threshold and om.size() > 1000
    assert bits_equal(lc.remap(*lc.map_words(case), frames[0]), ctx.front_end_u8(frames[0]))     # and the direct statement
    ctx.close()


# ---- a model changed on a live context ---------------------------------------------------------------------------------
ZERO = (0.0,) * 5
FINITE = "set_undistort: K4 and D5 must be finite"
POSITIVE = "set_undistort: focal lengths must be positive"
NO_MODEL_U8 = "front_end_u8: no distortion model set (rebvio_hip_set_undistort)"
NO_MODEL_PX = "front_end_px: no distortion model set (rebvio_hip_set_undistort)"


def _models(cols, rows):
    """A (fx != fy, barrel), B (pincushion, reads the border), no model, A again"""
    a = lc.at_size(lc.CAMERAS["euroc-quarter"], cols, rows)
    b = lc.at_size(lc.CAMERAS["pincushion-150-140"], cols, rows)
    return [a, b, a[:6] + (ZERO,), a]


def test_a_model_changed_on_a_live_context(B, small_stream):
    """Model A, model B, all-zero D5, A again on one context (set_undistort keeps the map's buffer from A to B, gives it back at
    the all-zero call and allocates it again): after each change one front_end_u8 and one detect_u8_host equal those of a fresh
    context that was given that model alone. The threshold servo is off (gain 0), so a detection does not depend on the frames
    detected before it; the test below runs the servo against the oracle. After the all-zero call front_end_u8 is refused
    with -3."""
    frames, cam = small_stream
    models = _models(cam.width, cam.height)
    kw = dict(KW_TRACK, gain=0.0)
    live = B.Context(params_for(B, cam, **kw))
    for k, case in enumerate(models):
        set_model(live, case)
        fresh = B.Context(params_for(B, cam, **kw))
        if case[6] == ZERO:
            with pytest.raises(B.HipError) as e:
                live.front_end_u8(frames[k])
            assert str(e.value) == f"rebvio_hip error -3: {NO_MODEL_U8}"
        else:
            set_model(fresh, case)
            assert bits_equal(fresh.front_end_u8(frames[k]), live.front_end_u8(frames[k])), k
        gl, gf = live.detect_u8_host(frames[k], k * TS), fresh.detect_u8_host(frames[k], k * TS)
        assert gl.size() > 500
        assert_keylines_equal(gf.keylines(), gl.keylines(), what=f"model {k}")
        assert gf.threshold == gl.threshold
        gl.release()
        gf.release()
        fresh.close()
    live.close()


def test_a_model_changed_on_a_live_context_against_the_oracle(orc_mod, B, small_stream):
    """The same four models on one live context, its detections against the oracle's detection of the oracle's front end with the
    model in force at each frame (x3 alone under the all-zero model)."""
    frames, cam = small_stream
    models = _models(cam.width, cam.height)
    live = B.Context(params_for(B, cam, **KW_TRACK))
    orc = orc_mod.Oracle(params_for(orc_mod, cam, **KW_TRACK))
    for k, case in enumerate(models):
        set_model(live, case)
        und = frames[k].astype(np.float32) * np.float32(3.0) if case[6] == ZERO else orc.front_end_u8(frames[k], *lc.K4(case), lc.D5(case))
        om, gm = orc.detect(und, k * TS), live.detect_u8_host(frames[k], k * TS)
        assert_keylines_equal(om.keylines(), gm.keylines(), what=f"model {k}")
        assert om.threshold == gm.threshold
        gm.release()
    live.close()


def test_a_model_changed_between_two_pushes_of_the_streaming_driver(B, small_stream):
    """Eight frames through push_frame_u8 with the model changed between pushes (A for frames 0-1, B for 2-3, none for 4-5, A for
    6-7): every word of every record equals the per-pair API's (detect_u8_host + track_pair) with the same change at the same
    frame."""
    frames, cam = small_stream
    models = _models(cam.width, cam.height)
    n = 8
    stream = B.Context(params_for(B, cam, **KW_TRACK))
    got = []
    for k in range(n):
        if k % 2 == 0:
            set_model(stream, models[k // 2])
        out, nk = stream.push_frame_u8(frames[k], k * TS)
        if out.status >= 0:
            got.append(rec(out, nk))
    got.extend(rec(o, nk) for o, nk in stream.flush())
    stream.close()
    pairs = B.Context(params_for(B, cam, **KW_TRACK))
    maps, want = [], []
    for k in range(n):
        if k % 2 == 0:
            set_model(pairs, models[k // 2])
        maps.append(pairs.detect_u8_host(frames[k], k * TS))
        if len(maps) > 2:
            maps.pop(0).release()
        if k:
            want.append(rec(pairs.track_pair(maps[0], maps[1]), maps[1].size()))
    pairs.close()
    assert len(want) == n - 1
    same_records(want, got, "model changed mid-stream")
    assert any(w[-2] == 0 for w in want), [int(w[-2]) for w in want]      # pairs that tracked (status 0)


# ---- a batch whose lanes have different cameras ---------------------------------------------------------------------------
def test_batch_lanes_with_three_different_cameras(orc_mod, B, small_stream):
    """Three lanes, three lens models (fx != fy on lane 0, a planted border pixel's camera on lane 1, tangential terms only on lane
    2), 4 steps through the batched front end (k_front_end_u8_b gathers every lane through ITS map): every lane's records equal
    a stand-alone context's with that model, and equal the oracle's track of the oracle's detections behind the oracle's front
    end - the batch ABI hands out no map, so the newest map is held to the oracle through the record of the pair that ends at it
    and its keyline count."""
    from rebvio_amd import synth
    frames, cam = small_stream
    cols, rows = cam.width, cam.height
    npx = cols * rows
    cases = [lc.at_size(lc.CAMERAS["euroc-quarter"], cols, rows), lc.planted("sx=cols-1", cols, rows)[0],
             lc.at_size(lc.CAMERAS["tangential-only"], cols, rows)]
    streams = [frames[:4], synth.render_stream(cols, rows, 4, stream_id=1)[0], synth.render_stream(cols, rows, 4, stream_id=2)[0]]
    bat = B.Batch(params_for(B, cam, **KW_TRACK), 3)
    for lane, case in zip(bat.lanes, cases):
        set_model(lane, case)
    devs = [bat.lanes[s].upload_frames(streams[s]) for s in range(3)]
    got = [[] for _ in range(3)]
    for k in range(4):
        outs, nks = bat.push_u8_device([d + k * npx for d in devs], k * TS)
        for s in range(3):
            if outs[s].status >= 0:
                got[s].append(rec(outs[s], nks[s]))
    for outs, nks in bat.flush():
        for s in range(3):
            got[s].append(rec(outs[s], nks[s]))
    bat.close()
    for s, case in enumerate(cases):
        ctx = B.Context(params_for(B, cam, **KW_TRACK))
        set_model(ctx, case)
        dev = ctx.upload_frames(streams[s])
        alone = []
        for k in range(4):
            out, nk = ctx.push_frame_u8_device(dev + k * npx, k * TS)
            if out.status >= 0:
                alone.append(rec(out, nk))
        alone.extend(rec(o, nk) for o, nk in ctx.flush())
        ctx.close()
        assert len(alone) == 3
        same_records(alone, got[s], f"lane {s} against a stand-alone context")
        orc = orc_mod.Oracle(params_for(orc_mod, cam, **KW_TRACK))
        orc.set_sum_order("device")
        prev, want = None, []
        for k in range(4):
            m = orc.detect(orc.front_end_u8(streams[s][k], *lc.K4(case), lc.D5(case)), k * TS)
            if prev is not None:
                want.append(np.append(record_words(orc.track_pair(prev, m)), np.uint32(m.size())))
            prev = m
        same_records(want, got[s], f"lane {s} against the oracle")
    assert not np.array_equal(got[0][-1], got[1][-1])


# ---- refusals ---------------------------------------------------------------------------------------------------------------
K_OK, D_OK = (90.0, 85.0, 70.5, 50.25), (-0.2, 0.05, 1e-3, -1e-3, 0.01)


def _with(values, k, v):
    out = list(values)
    out[k] = v
    return out


# (K4, D5, text). A word that is not finite is refused first, wherever it stands (a NaN focal length is "not finite", not "not
# positive"); then the focal lengths. Both hold with an all-zero D5 too, which would otherwise only switch the model off.
SET_REFUSALS = (
    [(_with(K_OK, k, 0.0), D, POSITIVE) for k in (0, 1) for D in (D_OK, ZERO)]
    + [(_with(K_OK, k, -90.0), D, POSITIVE) for k in (0, 1) for D in (D_OK, ZERO)]
    + [(_with(K_OK, k, np.nan), D, FINITE) for k in (0, 1) for D in (D_OK, ZERO)]
    + [(_with(K_OK, k, bad), D_OK, FINITE) for k in range(4) for bad in (np.nan, np.inf, -np.inf)]
    + [(K_OK, _with(D_OK, k, bad), FINITE) for k in range(5) for bad in (np.nan, np.inf, -np.inf)]
    + [(_with(K_OK, 0, -1.0), _with(D_OK, 4, np.nan), FINITE),          # both apply: the word that is not finite wins
       (_with(_with(K_OK, 0, 0.0), 3, np.inf), ZERO, FINITE),
       (_with(_with(K_OK, 0, 0.0), 1, np.nan), D_OK, FINITE)])


class LensScene:
    def __init__(self, B, cols, rows):
        self.B = B
        self.ctx, self.bare = context(B, cols, rows), context(B, cols, rows)
        self.case = lc.at_size(lc.CAMERAS["pincushion-150-140"], cols, rows)
        set_model(self.ctx, self.case)
        self.frame = noise_frames(cols, rows, 1, 21)[0]
        self.rgb = np.ascontiguousarray(np.repeat(self.frame[..., None], 3, -1))
        self.out = np.zeros((rows, cols), np.float32)
        self.before = self.ctx.front_end_u8(self.frame)

    def close(self):
        self.ctx.close()
        self.bare.close()


def test_refusals(B):
    """rebvio_hip_set_undistort and the two front-end entries, in the table style of support.assert_refused: the return code,
    the whole rebvio_hip_last_error text, nothing allocated, and the model set before still in force - one front_end_u8 after
    every refused call gives the bits it gave before."""
    fp = C.POINTER(C.c_float)
    L = B.lib()
    live = B.test_live_resources()
    scene = LensScene(B, 96, 64)

    def set_call(K, D):
        k, d = np.array(K, np.float32), np.array(D, np.float32)
        return lambda s: L.rebvio_hip_set_undistort(s.ctx.h, k.ctypes.data_as(fp), d.ctypes.data_as(fp))

    for K, D, text in SET_REFUSALS:
        assert_refused(scene, set_call(K, D), -3, text)
        assert bits_equal(scene.before, scene.ctx.front_end_u8(scene.frame)), (K, D)
    assert_refused(scene, lambda s: s.ctx.set_undistort(0.0, 85.0, 70.5, 50.25, list(D_OK)), -3, POSITIVE)      # through the binding
    # the front end without a model; front_end_px checks its frame and format first, then its output, then the model
    out = scene.out.ctypes.data_as(fp)
    frame, rgb = scene.frame.ctypes.data_as(C.c_void_p), scene.rgb.ctypes.data_as(C.c_void_p)
    assert_refused(scene, lambda s: L.rebvio_hip_front_end_u8(s.bare.h, frame, out), -3, NO_MODEL_U8)
    assert_refused(scene, lambda s: s.bare.front_end_u8(s.frame), -3, NO_MODEL_U8)
    assert_refused(scene, lambda s: L.rebvio_hip_front_end_px(s.bare.h, rgb, 0, RGB8, out), -3, NO_MODEL_PX)
    assert_refused(scene, lambda s: s.bare.front_end_px(s.rgb, RGB8), -3, NO_MODEL_PX)
    assert_refused(scene, lambda s: L.rebvio_hip_front_end_px(s.bare.h, rgb, 0, RGB8, None), -3, "front_end_px: null output")
    L.rebvio_hip_front_end_px(scene.bare.h, rgb, 0, 99, None)
    assert "unknown pixel format" in L.rebvio_hip_last_error().decode()
    assert not scene.out.any()                                       # a refused call writes nothing
    # a model switched off: refused again, and the refusal leaves it off; set again: the same bits as before
    scene.ctx.set_undistort(*K_OK, list(ZERO))
    assert_refused(scene, lambda s: L.rebvio_hip_front_end_u8(s.ctx.h, frame, out), -3, NO_MODEL_U8)
    assert_refused(scene, set_call(_with(K_OK, 1, 0.0), ZERO), -3, POSITIVE)
    assert_refused(scene, lambda s: L.rebvio_hip_front_end_u8(s.ctx.h, frame, out), -3, NO_MODEL_U8)
    set_model(scene.ctx, scene.case)
    assert bits_equal(scene.before, scene.ctx.front_end_u8(scene.frame))
    scene.close()
    assert B.test_live_resources() == live
