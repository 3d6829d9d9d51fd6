"""The stereo prior on the GPU (rebvio_hip_map_fuse_stereo*, k_stereo_prior).

Left maps are crafted through rebvio_hip_map_upload (a context of keylines_max = n detects exactly n keylines on a checkerboard
frame; the upload then replaces them). Right maps are detected ones - their mask is the detector's - or, for the planted cases,
written by hand through the upload and rebvio_hip_test_map_set_mask. Every word the device leaves - rho, sigma_rho, the outcome and
winner words, the counts - is compared with the host hook (rebvio_hip_test_stereo_prior_host, the same statements in index order,
the window's cells one by one), which tests/test_stereo_prior.py holds against the numpy restatement of the header. Every
comparison is equality.

The window of a keyline is ceil(d_max) - floor(d_min) + 3 cells wide before clipping, so 3 is the narrowest one an option can ask
for; a window of 1 cell comes from clipping at the image's first column (the planted case "one_cell"). Both are run, besides 15, 16,
17 (around the 16 lanes that serve a keyline) and 67 (the default: five steps of the lanes)."""
import ctypes as C

import numpy as np
import pytest

import stereo_prior_cases as SC
import stereo_prior_ref as R
from conftest import params_for
from support import B, refusal_scene  # noqa: F401
from support import DEAD_MAP, assert_refused
from support import F32, KW_TRACK, assert_keylines_equal, noise_frames, oracle_fusion, rec, same_records, vision_only_fusion, words

pytestmark = pytest.mark.gpu

MID_FIELDS = ("Vg", "P_Vg", "F", "sigma_rho_min", "Xv", "W_Xv", "Xgv")
BASELINE = 0.2


def checker(rows, cols, shift=0):
    """6-pixel checkerboard: 299 keylines at 32x32 with the threshold below, enough for maps of 257"""
    y, x = np.mgrid[0:rows, 0:cols]
    return (((((x + shift) // 6) + (y // 6)) % 2) * 200 + 20).astype(np.uint8)


def sized_ctx(B, n, rows=32, cols=32):
    from rebvio_amd import synth
    cam = synth.Camera.for_size(cols, rows)
    return B.Context(params_for(B, cam, keylines_ref=max(1, n - 1), keylines_max=max(1, n), threshold=0.001, gain=0.0,
                                global_min_matches_threshold=1))


def sized_map(ctx, n, ts=0, shift=0):
    rows, cols = ctx.rows, ctx.cols
    m = ctx.detect_u8(checker(rows, cols, shift) if n else np.full((rows, cols), 128, np.uint8), ts)
    assert m.size() == n, (m.size(), n)
    return m


def right_tables(mr):
    """what a right map holds, as the hook takes it"""
    return mr.keylines(), mr.mask()


def check(B, ml, mr, kl, opts, entry="sync", what=""):
    """upload kl into the left map, fuse mr through `entry`, compare everything with the hook; -> the counts tuple"""
    ctx = ml.ctx
    ml.upload(kl)
    back = ml.keylines()                                  # what the map holds (`id` is not kept on the device)
    for f in ("pos", "gradient", "gradient_norm", "rho", "sigma_rho", "matches"):
        assert back[f].tobytes() == kl[f].tobytes(), f
    kr, mask = right_tables(mr)
    before = (kr.tobytes(), mask.tobytes())
    want_c, want_kl, want_oc, want_win = B.stereo_prior_host(ctx.rows, ctx.cols, ctx.p.fm, back, kr, mask, opts)
    if entry == "sync":
        got_c, got_oc, got_win = ml.fuse_stereo(mr, opts, want_outcome=True)
        assert np.array_equal(got_oc, want_oc), (what, np.flatnonzero(got_oc != want_oc)[:8], got_oc[got_oc != want_oc][:8],
                                                 want_oc[got_oc != want_oc][:8])
        assert np.array_equal(got_win, want_win), (what, np.flatnonzero(got_win != want_win)[:8])
    else:
        assert ml.fuse_stereo(mr, opts, queued=True) is None
        got_c = ctx.stereo_prior_last_counts()
    assert got_c.as_tuple() == want_c.as_tuple(), (what, entry, got_c.as_tuple(), want_c.as_tuple())
    assert_keylines_equal(want_kl, ml.keylines(), what=f"{what} ({entry})")
    kr2, mask2 = right_tables(mr)
    assert (kr2.tobytes(), mask2.tobytes()) == before, f"{what}: the right map is only read"
    return got_c.as_tuple()


@pytest.fixture(scope="module")
def wide(B):
    """two contexts of 257 keylines at 96x48: the left map to craft, and a right map as the detector leaves it"""
    cl, cr = sized_ctx(B, 257, rows=48, cols=96), sized_ctx(B, 257, rows=48, cols=96)
    ml, mr = sized_map(cl, 257), sized_map(cr, 257, shift=2)
    yield ml, mr
    cl.close()
    cr.close()


# ---- sizes, windows, contexts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 63, 64, 65, 257])
def test_left_sizes_around_the_sub_group_and_the_workgroup(B, n):
    cl, cr = sized_ctx(B, n), sized_ctx(B, 257)
    ml, mr = sized_map(cl, n), sized_map(cr, 257, shift=1)
    kr, _ = right_tables(mr)
    rng = np.random.default_rng(100 + n)
    for row_tol in (0, 1):
        opts = B.default_stereo_prior_opts(cl, baseline=BASELINE, d_max=32.0, row_tol=row_tol)
        kl = SC.left_from_right(rng, kr, 32, 32, n, cl.p.fm * BASELINE, d_hi=20.0)
        c = check(B, ml, mr, kl, opts, what=f"n={n} row_tol={row_tol}")
        assert c[0] == n and (n < 63 or (c[3] > 0 and c[2] > 10)), c
    cl.close()
    cr.close()


@pytest.mark.parametrize("row_tol", [0, 1])
@pytest.mark.parametrize("width,d_min,d_max", [(3, 5.0, 5.0), (15, 0.0, 12.0), (16, 0.0, 13.0), (17, 2.0, 15.5), (67, 0.0, 64.0)])
def test_window_widths(B, wide, width, d_min, d_max, row_tol):
    ml, mr = wide
    assert int(np.ceil(d_max)) - int(np.floor(d_min)) + 3 == width
    kr, _ = right_tables(mr)
    rng = np.random.default_rng(width + row_tol)
    kl = SC.left_from_right(rng, kr, 48, 96, 257, ml.ctx.p.fm * BASELINE, d_hi=d_max + 2.0)
    opts = B.default_stereo_prior_opts(ml.ctx, baseline=BASELINE, d_min=d_min, d_max=d_max, row_tol=row_tol)
    c = check(B, ml, mr, kl, opts, what=f"width {width}")
    assert c[2] > 5 or width == 3, c   # (d_min = d_max leaves one exact disparity: the three cells are walked, nothing passes)
    check(B, ml, mr, kl, opts, entry="queued", what=f"width {width}")


def test_maps_of_one_context_and_37x33(B):
    ctx = sized_ctx(B, 257, rows=33, cols=37)
    ml, mr = sized_map(ctx, 257, 0), sized_map(ctx, 257, 50000, shift=3)
    kr, _ = right_tables(mr)
    rng = np.random.default_rng(37)
    kl = SC.left_from_right(rng, kr, 33, 37, 257, ctx.p.fm * BASELINE, d_hi=25.0)
    counts = {}
    for e in ("sync", "queued"):
        for name, kw in (("plain", {}), ("options", dict(d_min=1.5, d_max=20.0, min_ux=0.3, sigma_px=1.0, gate_sigma=2.0, ambig_px=0.5,
                                                          cos_min=0.5, norm_tol=0.5, q_abs=0.3))):
            opts = B.default_stereo_prior_opts(ctx, baseline=BASELINE, **dict(dict(d_max=37.0), **kw))
            counts[e, name] = check(B, ml, mr, kl, opts, entry=e, what=f"37x33 {name}")
    assert counts["sync", "plain"] == counts["queued", "plain"] and counts["sync", "plain"][3] > 10, counts
    ctx.close()


def test_last_counts_follow_the_most_recent_fusion(B, wide):
    ml, mr = wide
    ctx = ml.ctx
    kr, _ = right_tables(mr)
    kl = SC.left_from_right(np.random.default_rng(5), kr, 48, 96, 257, ctx.p.fm * BASELINE)
    o = B.default_stereo_prior_opts(ctx, baseline=BASELINE)
    a = check(B, ml, mr, kl, o, entry="queued", what="first")
    far = B.default_stereo_prior_opts(ctx, baseline=BASELINE, d_min=90.0, d_max=96.0)
    b = check(B, ml, mr, kl, far, entry="queued", what="second")
    assert a[3] > 0 and a != b
    assert ctx.stereo_prior_last_counts().as_tuple() == b                    # read twice
    c = check(B, ml, mr, kl, o, entry="sync", what="third")
    assert ctx.stereo_prior_last_counts().as_tuple() == c == a
    fresh = sized_ctx(B, 3)
    assert fresh.stereo_prior_last_counts().as_tuple() == (0,) * 8           # nothing yet
    fresh.close()


# ---- planted cases (tests/test_stereo_prior.py holds their outcomes against the hook and the restatement) ---------------------------
def test_planted_cases(B):
    n_left, n_right = 16, 64
    made = {}
    for name, rows, cols, fm, left, right, mask, opts, want, want_win in SC.planted_cases():
        if (rows, cols) not in made:
            from rebvio_amd import synth
            cam = synth.Camera(cols, rows, fm, cols / 2.0, rows / 2.0)
            kw = dict(threshold=0.001, gain=0.0, global_min_matches_threshold=1)
            cl = B.Context(params_for(B, cam, keylines_ref=n_left - 1, keylines_max=n_left, **kw))
            cr = B.Context(params_for(B, cam, keylines_ref=n_right - 1, keylines_max=n_right, **kw))
            made[rows, cols] = (cl, cr, sized_map(cl, n_left), sized_map(cr, n_right))
        cl, cr, ml, mr = made[rows, cols]
        assert cl.p.fm == fm and len(left) <= n_left and len(right) <= n_right
        kl = SC.keylines(n_left)
        kl["gradient_norm"] = 0.0                              # the padding is unusable
        kl[:len(left)] = left
        kr = SC.keylines(n_right)
        kr["gradient_norm"] = 0.0                              # ... and no candidate
        kr[:len(right)] = right
        mr.upload(kr)
        mr.set_mask(np.where(mask < len(right), mask, -1))    # (a word behind the table's end cannot exist on the device)
        o = B.default_stereo_prior_opts(**opts)
        check(B, ml, mr, kl, o, what=name)
        ml.upload(kl)
        _, oc, win = ml.fuse_stereo(mr, o, want_outcome=True)
        assert list(oc[:len(want)]) == want and (oc[len(want):] == 3).all(), (name, list(oc))
        if want_win is not None:
            assert list(win[:len(want)]) == want_win, (name, list(win))
        check(B, ml, mr, kl, o, entry="queued", what=name)
    with pytest.raises(B.HipError) as e:
        mr.set_mask(np.full((mr.ctx.rows, mr.ctx.cols), n_right, np.int32))
    assert "error -3:" in str(e.value)
    for cl, cr, _, _ in made.values():
        cl.close()
        cr.close()


# ---- re-use, the envelope ----------------------------------------------------------------------------------------------------------
def test_sizes_257_3_0_257_in_one_context(B):
    ctx = sized_ctx(B, 257)
    mr = sized_map(ctx, 257, 0, shift=2)
    m_a = sized_map(ctx, 257, 50000)
    ctx.set_detection_mask(((m_a.mask() >= 0) & (m_a.mask() < 3)).astype(np.uint8))
    m_3 = ctx.detect_u8(checker(32, 32), 100000)
    ctx.set_detection_mask(None)
    m_0 = sized_map(ctx, 0, 150000)
    m_b = sized_map(ctx, 257, 200000)
    assert (m_3.size(), m_0.size()) == (3, 0)
    kr, _ = right_tables(mr)
    o = B.default_stereo_prior_opts(ctx, baseline=BASELINE, d_max=32.0)
    rng = np.random.default_rng(8)
    for what, m in (("257", m_a), ("3", m_3), ("0", m_0), ("257 again", m_b), ("3 again", m_3)):
        for e in ("sync", "queued"):
            c = check(B, m, mr, SC.left_from_right(rng, kr, 32, 32, m.size(), ctx.p.fm * BASELINE, d_hi=20.0), o, entry=e, what=what)
            assert c[0] == m.size()
    # a right map of 3 and of 0 keylines
    kl = SC.left_from_right(rng, m_3.keylines(), 32, 32, 257, ctx.p.fm * BASELINE, d_hi=20.0)
    assert check(B, m_a, m_3, kl, o, what="right of 3")[0] == 257
    assert check(B, m_a, m_0, kl, o, what="right of 0")[2:] == (0, 0, 0, 0, 0, 0)
    ctx.close()


def test_the_full_envelope_of_65536_keylines(B):
    frames = noise_frames(896, 640, 2, 3)      # a noise frame of this size holds more candidates than the envelope
    ctx = B.Context(B.default_params(640, 896, fm=500.0, cx=447.5, cy=319.5, keylines_ref=60000, keylines_max=65536))
    ml, mr = ctx.detect_u8(frames[0], 0), ctx.detect_u8(frames[1], 50000)
    assert ml.size() == 65536 and mr.size() == 65536
    kr, _ = right_tables(mr)
    kl = SC.left_from_right(np.random.default_rng(4), kr, 640, 896, 65536, 500.0 * BASELINE, d_hi=60.0)
    c = check(B, ml, mr, kl, B.default_stereo_prior_opts(ctx, baseline=BASELINE), what="65536 keylines")
    assert c[0] == 65536 and c[2] > 20000 and c[3] > 1000, c
    ctx.close()


# ---- refusals, resources, launches --------------------------------------------------------------------------------------------------
def test_refusals_minus_7_minus_10_and_minus_3(B, small_stream):
    frames, cam = small_stream
    ctx = B.Context(params_for(B, cam, **KW_TRACK))
    rctx = B.Context(params_for(B, cam, **KW_TRACK))
    maps = [ctx.detect_u8(frames[i], i * 50000) for i in range(4)]
    right = [rctx.detect_u8(frames[i], i * 50000) for i in range(2)]
    o = B.default_stereo_prior_opts(ctx, baseline=BASELINE)
    c, s = F32(np.cos(0.01)), F32(np.sin(0.01))
    Rn = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], F32)
    assert maps[0].fuse_stereo(right[0], o).seen > 0                      # a stream's first map, right after detection
    mid = ctx.track_pair_begin(maps[0], maps[1])
    ctx.track_pair_finish_async(maps[0], maps[1], *vision_only_fusion(mid), R_prior_next=Rn)
    ctx.track_pair_result()
    for call in (lambda: maps[1].fuse_stereo(right[1], o), lambda: maps[1].fuse_stereo(right[1], o, queued=True)):
        with pytest.raises(B.HipError) as e:
            call()
        assert "error -7:" in str(e.value) and "R_prior_next" in str(e.value), str(e.value)   # promised: rotated for the next pair
    with pytest.raises(B.HipError) as e:
        maps[0].fuse_stereo(right[0], o)                                                      # has served as an old map
    assert "error -7:" in str(e.value) and "old map" in str(e.value), str(e.value)
    assert maps[2].fuse_stereo(maps[0], o).candidates == maps[2].size()   # ... which does not keep it from being a RIGHT map
    # -3 with live maps: the right map, the options, a left map of another context through the queued entry
    L = B.lib()
    cnt = B.StereoPriorCounts()
    assert L.rebvio_hip_map_fuse_stereo(maps[3].h, None, o, C.byref(cnt), None, None) == -3
    assert L.rebvio_hip_map_fuse_stereo(maps[3].h, right[1].h, o, None, None, None) == -3
    assert L.rebvio_hip_map_fuse_stereo(maps[3].h, right[1].h, None, C.byref(cnt), None, None) == -3      # no baseline
    assert L.rebvio_hip_last_error().decode().startswith("map_fuse_stereo: baseline")
    assert L.rebvio_hip_map_fuse_stereo(maps[3].h, right[1].h, B.default_stereo_prior_opts(ctx, baseline=BASELINE, row_tol=2),
                                        C.byref(cnt), None, None) == -3
    assert L.rebvio_hip_map_fuse_stereo_async(ctx.h, maps[3].h, None, o) == -3
    assert L.rebvio_hip_map_fuse_stereo_async(rctx.h, maps[3].h, right[1].h, o) == -3
    assert "another context" in L.rebvio_hip_last_error().decode()
    small = sized_ctx(B, 16)
    ms = sized_map(small, 16)
    assert L.rebvio_hip_map_fuse_stereo(maps[3].h, ms.h, o, C.byref(cnt), None, None) == -3
    assert "rows x cols" in L.rebvio_hip_last_error().decode()
    assert L.rebvio_hip_map_fuse_stereo_async(ctx.h, maps[3].h, ms.h, o) == -3
    small.close()
    # -10: the right map's context is gone, then the left one's
    rctx.close()
    assert L.rebvio_hip_map_fuse_stereo(maps[3].h, right[1].h, o, C.byref(cnt), None, None) == -10
    assert "destroyed" in L.rebvio_hip_last_error().decode()
    assert L.rebvio_hip_map_fuse_stereo_async(ctx.h, maps[3].h, right[1].h, o) == -10
    assert maps[3].fuse_stereo(maps[2], o).candidates == maps[3].size()   # the left context still works
    ctx.close()
    assert L.rebvio_hip_map_fuse_stereo(maps[3].h, maps[2].h, o, C.byref(cnt), None, None) == -10
    for m in maps + right + [ms]:
        m.release()


def test_one_launch_per_call_and_one_allocation(B):
    """k_stereo_prior once per call whatever the maps hold; the first call gives the LEFT context one live resource (the counts,
    outcome and winner words) and no call after that anything; a refused call allocates nothing; the right map's context gets
    nothing; nothing is left after destroy"""
    live = B.test_live_resources()
    ctx, rctx = sized_ctx(B, 257), sized_ctx(B, 257)
    m, m0, mr = sized_map(ctx, 257, 0), sized_map(ctx, 0, 50000), sized_map(rctx, 257, shift=1)
    for x in (m, m0, mr):
        x.keylines()
    o = B.default_stereo_prior_opts(ctx, baseline=BASELINE, d_max=32.0)
    base = B.test_live_resources()
    with pytest.raises(B.HipError):
        m.fuse_stereo(mr, B.default_stereo_prior_opts(ctx, baseline=0.0))
    assert B.test_live_resources() == base
    ctx.profile(True)
    for k, (mm, kw) in enumerate(((m, {}), (m0, {}), (m, dict(queued=True)), (m, {}))):
        ctx.profile_reset()
        mm.fuse_stereo(mr, o, **kw)
        ctx.stereo_prior_last_counts()
        launches = {name: calls for name, (_, calls) in ctx.profile_read().items() if calls}
        assert launches == {"k_stereo_prior": 1}, (k, launches)
        assert B.test_live_resources() == base + 1, k
    ctx.profile(False)
    ctx.close()
    rctx.close()
    for x in (m, m0, mr):
        x.release()
    assert B.test_live_resources() == live


# ---- with the tracker -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stereo_runs(orc_mod):
    """the 192x144 stereo stream's 10 frames through the oracle, with the restatement fusing every frame's right map and without"""
    from rebvio_amd import synth
    left, right, cam = synth.render_stereo_stream(192, 144, 10, BASELINE)
    p = params_for(orc_mod, cam, **KW_TRACK)
    return left, right, cam, R.oracle_stream(orc_mod, p, left, right, BASELINE), R.oracle_stream(orc_mod, p, left, None, BASELINE)


def test_pipeline_through_track_pair_equals_oracle_plus_restatement(B, stereo_runs):
    """fusion between the pairs of rebvio_hip_track_pair, the right maps from a second, detect-only context: every word of every
    pair record, the counts and outcome words of every fusion and every keyline field of every left map equal the
    oracle-plus-restatement run"""
    left, right, cam, want, _ = stereo_runs
    ctx, rctx = B.Context(params_for(B, cam, **KW_TRACK)), B.Context(params_for(B, cam, **KW_TRACK))
    o = B.default_stereo_prior_opts(ctx, baseline=BASELINE)
    maps = [ctx.detect_u8(left[k], k * 50000) for k in range(10)]
    for k in range(10):
        mr = rctx.detect_u8(right[k], k * 50000)
        if k:
            pg = ctx.track_pair(maps[k - 1], maps[k])
            wo, wg = rec(want["records"][k - 1], want["sizes"][k - 1]), rec(pg, maps[k].size())
            assert np.array_equal(wo, wg), (k, np.flatnonzero(wo != wg)[:8])
        c, oc, _ = maps[k].fuse_stereo(mr, o, want_outcome=True)
        assert c.as_tuple() == R.counts_tuple(want["counts"][k]), (k, c.as_tuple(), want["counts"][k])
        assert np.array_equal(oc, want["outcomes"][k]), k
        assert_keylines_equal(want["keylines"][k], maps[k].keylines(), what=f"left map {k} after its fusion")
        mr.release()
    assert all(r.status == 0 for r in want["records"])
    with pytest.raises(B.HipError) as e:
        maps[8].fuse_stereo(maps[9], o)                                   # rebvio_hip_track_pair marks its old map
    assert "error -7:" in str(e.value) and "old map" in str(e.value), str(e.value)
    ctx.close()
    rctx.close()


def test_pipeline_through_the_split_api_with_the_queued_entry(orc_mod, B, stereo_runs):
    """the same through rebvio_hip_track_pair_begin / _finish_async, the fusion queued between _finish_async(k) and _begin(k + 1)
    and nothing waited for in between (the order rebvio::Rebvio uses); handed the oracle's own fusion results the halves reproduce
    the oracle-plus-restatement run: the first half's record, the second half's counters, the fusions' counts, the newest map.
    A right map stays unreleased until a later synchronising call on the left context has returned."""
    left, right, cam, want, _ = stereo_runs
    ctx, rctx = B.Context(params_for(B, cam, **KW_TRACK)), B.Context(params_for(B, cam, **KW_TRACK))
    o = B.default_stereo_prior_opts(ctx, baseline=BASELINE)
    maps = [ctx.detect_u8(left[k], k * 50000) for k in range(10)]
    rights = [rctx.detect_u8(right[0], 0)]
    maps[0].fuse_stereo(rights[0], o, queued=True)
    for k in range(1, 10):
        po = want["records"][k - 1]
        rights.append(rctx.detect_u8(right[k], k * 50000))
        mid = ctx.track_pair_begin(maps[k - 1], maps[k])                  # (synchronises: the right map of k - 1 has been read)
        rights[k - 1].release()
        if k > 1:
            assert ctx.track_pair_result() == (pp.klm_num, pp.kf_matches, pp.reg_num, pp.status), k
        for f in MID_FIELDS:
            assert np.array_equal(words(getattr(mid, f)), words(getattr(po, f))), (k, f)
        ctx.track_pair_finish_async(maps[k - 1], maps[k], *oracle_fusion(orc_mod, po))
        maps[k].fuse_stereo(rights[k], o, queued=True)
        if k in (1, 5, 9):
            assert ctx.stereo_prior_last_counts().as_tuple() == R.counts_tuple(want["counts"][k]), k
        pp = po
    assert ctx.track_pair_result() == (pp.klm_num, pp.kf_matches, pp.reg_num, pp.status)
    assert_keylines_equal(want["keylines"][9], maps[9].keylines(), what="newest map, split API with queued fusions")
    ctx.close()
    rctx.close()


def test_a_stream_without_a_stereo_call_is_unchanged(B, stereo_runs):
    """no stereo call: the records are the oracle's word for word"""
    left, _, cam, _, want = stereo_runs
    ctx = B.Context(params_for(B, cam, **KW_TRACK))
    maps = [ctx.detect_u8(left[k], k * 50000) for k in range(10)]
    got = [rec(ctx.track_pair(maps[k - 1], maps[k]), maps[k].size()) for k in range(1, 10)]
    same_records([rec(r, n) for r, n in zip(want["records"], want["sizes"])], got, "no stereo")
    assert_keylines_equal(want["keylines"][9], maps[9].keylines(), what="newest map without stereo")
    ctx.close()


# ---- the refusal table: every shared refusal with its code and whole text; which one wins when several apply ------

STEREO = "map_fuse_stereo"
_so = lambda s, **kw: s.B.default_stereo_prior_opts(s.ctx, baseline=0.1, **kw)
_queued = lambda s, m, r: s.B.lib().rebvio_hip_map_fuse_stereo_async(s.other.h, m.h, r.h, _so(s))
REFUSED = {
    "queued: left map of another context": (lambda s: _queued(s, s.m, s.m2), -3, "map_fuse_stereo_async: left map of another context"),
    "queued: wins: a destroyed right map over another context": (lambda s: _queued(s, s.m, s.dm), -10, DEAD_MAP),
    "destroyed left map": (lambda s: s.dm.fuse_stereo(s.m, _so(s)), -10, DEAD_MAP),
    "destroyed right map": (lambda s: s.m.fuse_stereo(s.dm, _so(s)), -10, DEAD_MAP),
    "gate_sigma": (lambda s: s.m.fuse_stereo(s.m2, _so(s, gate_sigma=0.0)), -3, f"{STEREO}: gate_sigma must be > 0"),
    "q_abs": (lambda s: s.m.fuse_stereo(s.m2, _so(s, q_abs=-1.0)), -3, f"{STEREO}: q_abs must be >= 0"),
    "wins: a destroyed map over an option": (lambda s: s.m.fuse_stereo(s.dm, _so(s, q_abs=-1.0)), -10, DEAD_MAP),
    "wins: sigma_px over gate_sigma": (lambda s: s.m.fuse_stereo(s.m2, _so(s, sigma_px=0.0, gate_sigma=0.0)), -3,
                                       f"{STEREO}: sigma_px must be > 0 and finite"),
    "wins: gate_sigma over ambig_px": (lambda s: s.m.fuse_stereo(s.m2, _so(s, gate_sigma=0.0, ambig_px=-1.0)), -3,
                                       f"{STEREO}: gate_sigma must be > 0"),
    "wins: norm_tol over q_abs": (lambda s: s.m.fuse_stereo(s.m2, _so(s, norm_tol=-1.0, q_abs=-1.0)), -3, f"{STEREO}: norm_tol must be >= 0"),
    "wins: q_abs over reserved": (lambda s: s.m.fuse_stereo(s.m2, _so(s, q_abs=-1.0, reserved=2)), -3, f"{STEREO}: q_abs must be >= 0"),
}

@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusal_table(refusal_scene, case):
    """every refusal of the table with its return code and its whole rebvio_hip_last_error text; nothing is allocated"""
    assert_refused(refusal_scene, *REFUSED[case])
