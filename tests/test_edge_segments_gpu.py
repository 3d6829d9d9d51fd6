"""Straight segments of the edge polylines (rebvio_hip_map_edge_segments) on the GPU.

Maps are crafted through rebvio_hip_map_upload (a context of keylines_max = n detects exactly n keylines on a busy frame; the upload
then replaces them) and the device's result is compared with the library's host hook on the keylines downloaded from the map - the same
per-point statements, compiled for the host, which tests/test_edge_segments.py holds against the restatement of
tests/edge_segments_ref.py - and on a detected, tracked map with the restatement itself. Record bytes and counts: every comparison is
equality."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from conftest import params_for
from edge_chains_ref import KERNELS_CHAINS, KERNELS_POLY, WIDE, rounds_of
from edge_segments_ref import (KERNELS_SEG, LINE_SEGMENT_DTYPE, LOOSE, assert_segments_equal, keylines_on_paths, np_segments, opts_of,
                               planted_cases, seg_launches, straight, with_depths)
from support import B, refusal_scene  # noqa: F401
from support import DEAD_MAP, F32, KW_TRACK, assert_refused, noise_frames, vision_only_fusion

pytestmark = pytest.mark.gpu

W, H = 160, 120
POSE = (np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]], F32), np.array([0.5, -1.25, 2.0], F32), F32(1.5))


@functools.lru_cache(maxsize=None)
def stream(n=3):
    from rebvio_amd import synth
    return synth.render_stream(W, H, n)


def sized_ctx(B, n):
    """a context whose detections of the stream's frames hold exactly n >= 1 keylines: keylines_max = n truncates them"""
    _, cam = stream()
    return B.Context(params_for(B, cam, keylines_ref=max(1, n - 1), keylines_max=n, global_min_matches_threshold=1))


def sized_map(B, ctx, n, frame=1):
    m = ctx.detect_u8(stream()[0][frame] if n else np.full((H, W), 128, np.uint8), 0)
    assert m.size() == n, (m.size(), n)
    return m


def padded(kl, n):
    """kl with unlinked keylines behind it up to n: they are chains of one member, which no option here keeps"""
    out = np.zeros(n, kl.dtype)
    out[:len(kl)] = kl
    out["id_prev"][len(kl):] = out["id_next"][len(kl):] = -1
    out["id"] = np.arange(n)
    return out


def upload(m, kl):
    m.upload(kl)
    back = m.keylines()
    for f in ("id_prev", "id_next", "pos_img", "rho", "sigma_rho", "matches"):      # what the entry reads
        assert back[f].tobytes() == kl[f].tobytes(), f
    return back


def check(B, ctx, m, kl, kw, what, pose=POSE, cap=None):
    """device == hook on the map's own keylines; returns the counts"""
    opts = opts_of(B, kw)
    got = m.edge_segments(opts, pose, cap)
    assert_segments_equal(got, B.edge_segments_host(ctx.p.fm, kl, opts, pose, cap), what)
    return got[1].as_dict()


# ---- the planted cases ---------------------------------------------------------------------------------------------------------------
def test_every_planted_case(B):
    """the cases tests/test_edge_segments.py states by hand, each padded to one map size, in ONE context: one after another they also
    leave each other's far / nxt words behind"""
    ctx = sized_ctx(B, 300)
    m = sized_map(B, ctx, 300)
    for name, kl, kw, cap in planted_cases(B.KEYLINE_DTYPE):
        if name == "empty":
            continue
        kw = dict(kw, min_chain_length=max(2, kw.get("min_chain_length", 8)))
        back = upload(m, padded(kl, 300))
        cnt = check(B, ctx, m, back, kw, name, cap=cap)
        want = np_segments(back, ctx.p.fm, pose=POSE, **kw)      # and the restatement: the planted maps are small
        assert_segments_equal(m.edge_segments(opts_of(B, kw), POSE, cap), want, name + " (restatement)", cap)
        assert cnt["points"] == len(kl), (name, cnt)
    ctx.close()
    ctx = sized_ctx(B, 1)
    m0 = sized_map(B, ctx, 0)
    got = m0.edge_segments()
    assert len(got[0]) == 0 and not any(got[1].as_dict().values())
    ctx.close()


# ---- wave and workgroup boundaries --------------------------------------------------------------------------------------------------
LENGTHS = (63, 64, 65, 255, 256, 257)


def boundary_paths(kind):
    paths, y = [], -50.0
    for n in LENGTHS:
        if kind == "straight":      # a wobble below the tolerance: no split, every wave's winner of the line into one word
            paths.append([(-70.0 + 0.5 * i, y + 0.3 * math.sin(1.7 * i)) for i in range(n)])
        else:                       # an arc with a ripple: splits at every level, vertices in every lane
            paths.append([(90.0 * math.cos(a) + 0.4 * math.sin(2.3 * i), 90.0 * math.sin(a) + y) for i, a in enumerate(np.linspace(0.0, 2.5, n))])
        y += 8.0
    return paths


@pytest.mark.parametrize("kind", ["straight", "bent"])
def test_lines_of_63_to_257_points(B, kind):
    """lines of 63, 64, 65, 255, 256 and 257 points one behind the other (960 points): the second line starts in lane 63 of wave 0;
    straight, each is ONE segment that spans waves and (from the fourth on) workgroups - its maximum comes together from several
    atomics and its fit runs 16 lanes over up to 17 members each; bent, segments start and end in every lane"""
    n = sum(LENGTHS)
    ctx = sized_ctx(B, n)
    m = sized_map(B, ctx, n)
    kl = upload(m, with_depths(keylines_on_paths(B.KEYLINE_DTYPE, boundary_paths(kind))))
    cnt = check(B, ctx, m, kl, dict(LOOSE), kind)
    print(kind, cnt)
    if kind == "straight":
        got = m.edge_segments(opts_of(B, LOOSE))[0]
        assert [int(s["points"]) for s in got] == list(LENGTHS) and list(got["first_point"]) == list(np.cumsum((0,) + LENGTHS[:-1]))
        assert cnt["rounds_used"] == 0 and (got["max_dev2"] > 0).all() and (got["flags"] == 1).all()
    else:
        assert cnt["rounds_used"] >= 4 and cnt["unresolved"] == 0 and cnt["kept"] > 60
    check(B, ctx, m, kl, dict(min_chain_length=8), kind + ", default options")
    ctx.close()


def test_1000_two_point_segments_in_a_row(B):
    """1001 points on a half circle of radius 400 000 px (785 px apart; the sagitta of two steps is 1.97 px, 60 ulp of a coordinate):
    the splits are balanced, 10 levels, and every point ends as a vertex - 1000 segments of two points. In the last splitting round
    the segments have one or two interior points each: one atomic per (wave, segment), from lanes next to each other; in the
    measuring pass behind it no segment has an interior point left and no atomic is issued at all"""
    n = 1001
    ctx = sized_ctx(B, n)
    m = sized_map(B, ctx, n)
    pts = [(400000.0 * math.cos(a), 400000.0 * math.sin(a)) for a in np.linspace(0.0, math.pi, n)]
    kl = upload(m, with_depths(keylines_on_paths(B.KEYLINE_DTYPE, [pts])))
    cnt = check(B, ctx, m, kl, dict(LOOSE), "zig-zag 1001")
    print(cnt)
    assert (cnt["segments_all"], cnt["kept"], cnt["unresolved"], cnt["rounds_used"]) == (1000, 1000, 0, 10)
    cnt = check(B, ctx, m, kl, dict(LOOSE, max_rounds=3), "zig-zag 1001, three rounds")
    assert cnt["rounds_used"] == 3 and cnt["segments_all"] == 8 and cnt["unresolved"] == 8
    ctx.close()


def test_the_full_envelope_of_65536_points(B):
    """keylines_max = 65 536: ONE straight line of 65 536 points (one segment: every wave's winner into one word, a fit of 4096 members
    per lane), then a zig-zag on an arc over all of them (16 levels of splits across 256 workgroups)"""
    frame = noise_frames(896, 640, 1, 3)[0]      # a noise frame of this size holds more candidates than the envelope
    ctx = B.Context(B.default_params(640, 896, fm=500.0, cx=447.5, cy=319.5, keylines_ref=60000, keylines_max=65536))
    m = ctx.detect_u8(frame, 0)
    n = m.size()
    assert n == 65536, n
    i = np.arange(n)
    kl = with_depths(keylines_on_paths(B.KEYLINE_DTYPE, [list(zip(i / 64.0 - 400.0, 0.25 * (i / 64.0) + 0.3 * np.sin(0.37 * i)))]))
    kl = upload(m, kl)
    cnt = check(B, ctx, m, kl, dict(LOOSE), "one line of 65 536")
    seg = m.edge_segments(opts_of(B, LOOSE))[0]
    assert (cnt["segments_all"], cnt["kept"], cnt["rounds_used"], cnt["points"], cnt["lines"]) == (1, 1, 0, n, 1)
    assert (int(seg[0]["points"]), int(seg[0]["flags"])) == (n, 1) and 0 < seg[0]["max_dev2"] < 1.0
    ang = np.linspace(0.0, 1.0, n)
    kl = with_depths(keylines_on_paths(B.KEYLINE_DTYPE, [list(zip(32768.0 * np.sin(ang), 32768.0 * (1 - np.cos(ang)) + 3.0 * (i % 2)))]))
    kl = upload(m, kl)
    cnt = check(B, ctx, m, kl, dict(LOOSE), "zig-zag of 65 536")
    print(cnt)
    # (where the arc's sagitta falls below the zig-zag's 3 px the nearly tied winners peel a segment from its front: 16 rounds do not
    # resolve it - the host hook says 1755 segments, 206 of them unresolved)
    assert cnt["rounds_used"] == 16 and cnt["segments_all"] > 1000 and cnt["unresolved"] > 0
    ctx.close()


# ---- re-use, launches, resources ------------------------------------------------------------------------------------------------------
def reuse_maps(B, ctx):
    """maps of 1000, 3, 0 and 1000 keylines in one context of keylines_max 1000: the 3 through a detection mask that lets only the
    pixels of the first three keylines through, the 0 from a blank frame"""
    frames, _ = stream()
    m_a = ctx.detect_u8(frames[1], 0)
    assert m_a.size() == 1000
    ctx.set_detection_mask(((m_a.mask() >= 0) & (m_a.mask() < 3)).astype(np.uint8))
    m_3 = ctx.detect_u8(frames[1], 50000)
    ctx.set_detection_mask(None)
    m_0 = ctx.detect_u8(np.full((H, W), 128, np.uint8), 100000)
    m_b = ctx.detect_u8(frames[2], 150000)
    assert (m_3.size(), m_0.size(), m_b.size()) == (3, 0, 1000), (m_3.size(), m_0.size(), m_b.size())
    return m_a, m_3, m_0, m_b


def reuse_keylines(B):
    bent = [(200.0 * math.cos(a) - 150.0, 200.0 * math.sin(a) + 2.0 * (i % 3)) for i, a in enumerate(np.linspace(0.0, 1.2, 700))]
    kl_a = with_depths(keylines_on_paths(B.KEYLINE_DTYPE, [bent, straight(300)]))
    kl_3 = with_depths(keylines_on_paths(B.KEYLINE_DTYPE, [[(0.0, 0.0), (2.0, 5.0), (4.0, 0.0)]]))
    kl_b = with_depths(keylines_on_paths(B.KEYLINE_DTYPE, [straight(500), bent[:500]]))
    return kl_a, kl_3, kl_b


def test_reuse_in_one_context_leaves_nothing_stale(B):
    """sizes 1000, then 3, then 0, then 1000 with other lines: every call's result is its own map's (far, nxt and the round words of
    the call in front lie in the same scratch)"""
    ctx = sized_ctx(B, 1000)
    m_a, m_3, m_0, m_b = reuse_maps(B, ctx)
    kl_a, kl_3, kl_b = (upload(m, kl) for m, kl in zip((m_a, m_3, m_b), reuse_keylines(B)))
    for what, m, kl in (("1000", m_a, kl_a), ("3", m_3, kl_3), ("0", m_0, m_0.keylines()), ("1000 again", m_b, kl_b), ("3 again", m_3, kl_3),
                        ("1000 a third time", m_a, kl_a)):
        cnt = check(B, ctx, m, kl, dict(LOOSE), what)
        assert cnt["points"] == len(kl) and (len(kl) == 0 or cnt["kept"] >= 2), (what, cnt)
    ctx.close()


def test_the_entry_launches_what_the_header_documents_and_holds_one_allocation(B):
    """R + 8 launches of the polylines and 2 * max_rounds + 5 of the segments, the same at n = 0, 3 and 1000; one live resource more
    after the first call (behind the chains' own), none per call, none left after destroy; a context that has run all of it still
    fits profile_read"""
    live = B.test_live_resources()
    ctx = sized_ctx(B, 1000)
    m_a, m_3, m_0, m_b = reuse_maps(B, ctx)
    upload(m_a, reuse_keylines(B)[0])
    for m in (m_a, m_3, m_0):
        m.keylines()
    m_0.edge_polylines()      # the chains' scratch: not this entry's
    base = B.test_live_resources()
    R = rounds_of(1000)
    ctx.profile(True)
    for max_rounds in (16, 1, 32):
        want = dict({k: 1 for k in KERNELS_CHAINS + KERNELS_POLY + KERNELS_SEG}, k_chain_round=R, k_seg_far=max_rounds + 1, k_seg_split=max_rounds)
        for m in (m_0, m_3, m_a):
            ctx.profile_reset()
            m.edge_segments(opts_of(B, dict(LOOSE, max_rounds=max_rounds)))
            launches = {name: calls for name, (_, calls) in ctx.profile_read().items() if calls}
            assert launches == want and sum(launches.values()) == R + 8 + seg_launches(max_rounds), (m.size(), launches)
            assert B.test_live_resources() == base + 1
    ctx.profile_reset()
    ctx.track_pair(m_a, m_b)
    m_b.edge_segments()
    m_b.point_cloud()
    names = ctx.profile_read()
    assert set(KERNELS_SEG) <= set(names) and len(names) < 128, len(names)
    ctx.profile(False)
    ctx.close()
    for m in (m_a, m_3, m_0, m_b):
        m.release()
    assert B.test_live_resources() == live


# ---- a detected, tracked map ------------------------------------------------------------------------------------------------------------
def test_a_tracked_map_against_the_restatement(B, small_stream):
    """detection and four tracked pairs on the device, then the segments of the last map against the restatement and the hook"""
    frames, cam = small_stream
    ctx = B.Context(params_for(B, cam, **KW_TRACK))
    maps = [ctx.detect_u8(frames[k], k * 50000) for k in range(5)]
    for k in range(4):
        ctx.track_pair(maps[k], maps[k + 1])
    kl = maps[4].keylines()
    for kw, pose in ((dict(flt=(1, 0.5, 1e-3, 20.0)), POSE), (dict(flt=WIDE), None), (dict(flt=WIDE, tol=0.7, min_points=4), POSE)):
        want = np_segments(kl, ctx.p.fm, pose=pose, **kw)
        print(kw, want[1])
        assert_segments_equal(maps[4].edge_segments(opts_of(B, kw), pose), want, kw)
        assert_segments_equal(B.edge_segments_host(ctx.p.fm, kl, opts_of(B, kw), pose), want, (kw, "hook"))
        assert want[1]["kept"] > (3 if kw["flt"] != WIDE else 50) and want[1]["unresolved"] == 0
    ctx.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_minus_7_and_minus_10(B, small_stream):
    frames, cam = small_stream
    ctx = B.Context(params_for(B, cam, **KW_TRACK))
    maps = [ctx.detect_u8(frames[i], i * 50000) for i in range(3)]
    c, s = F32(np.cos(0.01)), F32(np.sin(0.01))
    Rn = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], F32)
    mid = ctx.track_pair_begin(maps[0], maps[1])
    ctx.track_pair_finish_async(maps[0], maps[1], *vision_only_fusion(mid), R_prior_next=Rn)
    ctx.track_pair_result()
    with pytest.raises(B.HipError) as e:
        maps[1].edge_segments()
    assert "error -7:" in str(e.value) and "R_prior_next" in str(e.value), str(e.value)
    check(B, ctx, maps[0], maps[0].keylines(), dict(flt=WIDE), "the pair's old map carries no promise")
    mid = ctx.track_pair_begin(maps[1], maps[2], R_prior=Rn)
    ctx.track_pair_finish_async(maps[1], maps[2], *vision_only_fusion(mid))
    ctx.track_pair_result()
    check(B, ctx, maps[1], maps[1].keylines(), dict(flt=WIDE), "after the next begin")
    L = B.lib()
    cnt = B.SegmentCounts()
    ctx.close()
    assert L.rebvio_hip_map_edge_segments(maps[1].h, None, None, None, 0, C.byref(cnt)) == -10
    assert "destroyed" in L.rebvio_hip_last_error().decode()
    for m in maps:
        m.release()


def _raw(s, opts=None, pose=None, cap=0, counts=True, m=None):
    cnt = s.B.SegmentCounts()
    buf = np.zeros(4, LINE_SEGMENT_DTYPE)
    return s.B.lib().rebvio_hip_map_edge_segments((m or s.m).h, opts, pose, buf.ctypes.data if cap == "buf" else None, 4 if cap == "buf" else cap,
                                                  C.byref(cnt) if counts else None)


# the refusal table: every refusal with its code and whole text; which one wins when several apply
REFUSED = {
    "null counts": (lambda s: _raw(s, counts=False), -3, "map_edge_segments: null counts"),
    "negative cap": (lambda s: _raw(s, cap=-1), -3, "map_edge_segments: cap_segments records need a segs buffer (cap_segments >= 0)"),
    "a cap without a buffer": (lambda s: _raw(s, cap=5), -3, "map_edge_segments: cap_segments records need a segs buffer (cap_segments >= 0)"),
    "negative tol": (lambda s: s.m.edge_segments(s.B.default_segment_opts(tol=-1.0)), -3, "map_edge_segments: tol and min_length must be >= 0"),
    "NaN min_length": (lambda s: s.m.edge_segments(s.B.default_segment_opts(min_length=float("nan"))), -3,
                       "map_edge_segments: tol and min_length must be >= 0"),
    "min_points 1": (lambda s: s.m.edge_segments(s.B.default_segment_opts(min_points=1)), -3, "map_edge_segments: min_points must be >= 2"),
    "max_rounds 0": (lambda s: s.m.edge_segments(s.B.default_segment_opts(max_rounds=0)), -3, "map_edge_segments: max_rounds must be in 1..32"),
    "max_rounds 33": (lambda s: s.m.edge_segments(s.B.default_segment_opts(max_rounds=33)), -3, "map_edge_segments: max_rounds must be in 1..32"),
    "min_chain_length 0": (lambda s: s.m.edge_segments(s.B.default_segment_opts(poly=dict(min_chain_length=0))), -3,
                           "map_edge_segments: min_chain_length must be >= 1"),
    "the filter": (lambda s: s.m.edge_segments(s.B.default_segment_opts(poly=dict(filter=dict(rho_min=-1.0)))), -3,
                   "map_edge_segments: filter rho_min must be > 0"),
    "NaN in the pose": (lambda s: s.m.edge_segments(None, s.B.cloud_pose(t=[0, float("nan"), 0])), -3, "map_edge_segments: NaN in the pose"),
    "a destroyed map": (lambda s: s.dm.edge_segments(), -10, DEAD_MAP),
    "wins: the options over a destroyed map": (lambda s: s.dm.edge_segments(s.B.default_segment_opts(min_points=0)), -3,
                                               "map_edge_segments: min_points must be >= 2"),
    "wins: null counts over the options": (lambda s: _raw(s, s.B.default_segment_opts(tol=-1.0), counts=False), -3, "map_edge_segments: null counts"),
}
@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusal_table(refusal_scene, case):
    """every refusal of the table with its return code and its whole rebvio_hip_last_error text; nothing is allocated"""
    assert_refused(refusal_scene, *REFUSED[case])
