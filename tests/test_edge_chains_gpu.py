"""Edge chains and polylines (rebvio_hip_map_edge_chains / rebvio_hip_map_edge_polylines) on the GPU.

Maps are crafted through rebvio_hip_map_upload (a context of keylines_max = n detects exactly n keylines on a busy frame; the upload
then replaces them) and the device's result is compared with the numpy restatement of tests/edge_chains_ref.py - a sequential walk,
checked by hand in tests/test_edge_chains.py - applied to the keylines downloaded from the map. Integers and record bytes: every
comparison is equality."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import params_for
from edge_chains_ref import (DEFAULT_FILTER, KERNELS_CHAINS, KERNELS_POLY, WIDE, assert_chains_equal, assert_polylines_equal,
                             dirty_links, keylines_with_links, links_of_sequences, np_chains, np_polylines, planted_polyline_map,
                             rounds_of, shuffled_path)
from support import B  # noqa: F401
from support import F32, KW_TRACK, noise_frames, rec, same_records, vision_only_fusion

pytestmark = pytest.mark.gpu

W, H = 160, 120
POSE = (np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]], F32), np.array([0.5, -1.25, 2.0], F32), F32(1.5))


@functools.lru_cache(maxsize=None)
def stream(w=W, h=H, n=3):
    from rebvio_amd import synth
    return synth.render_stream(w, h, n)


def sized_ctx(B, n):
    """a context whose detections of the stream's frames hold exactly n >= 1 keylines: keylines_max = n truncates them"""
    _, cam = stream()
    return B.Context(params_for(B, cam, keylines_ref=max(1, n - 1), keylines_max=n, global_min_matches_threshold=1))


def sized_map(B, ctx, n, frame=1):
    m = ctx.detect_u8(stream()[0][frame] if n else np.full((H, W), 128, np.uint8), 0)
    assert m.size() == n, (m.size(), n)
    return m


def upload_links(B, m, idp, idn, seed=0):
    kl = keylines_with_links(B.KEYLINE_DTYPE, idp, idn, seed)
    m.upload(kl)
    back = m.keylines()
    for f in ("id_prev", "id_next", "pos_img", "rho", "sigma_rho", "gradient_norm", "matches"):      # what the two entries read
        assert back[f].tobytes() == kl[f].tobytes(), f
    return back


def check_chains(m, kl, what):
    want = np_chains(kl["id_prev"], kl["id_next"])
    assert_chains_equal(m.edge_chains(), want, what)
    return want


def opts_of(B, flt, min_len):
    return B.default_polyline_opts(min_chain_length=min_len, filter=dict(zip(("min_matches", "max_rel_sigma", "rho_min", "rho_max"), flt)))


# ---- small sizes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 257, 300])
def test_small_sizes(B, n):
    """n = 0, 1 and 2; a path across a workgroup edge (n = 257: the link 255 > 256); a path in descending index order (n = 300)"""
    ctx = sized_ctx(B, max(n, 1))
    m = sized_map(B, ctx, n)
    cases = {0: [("empty", links_of_sequences(0))],
             1: [("single", links_of_sequences(1)), ("self link", (np.zeros(1, np.int32), np.zeros(1, np.int32))),
                 ("wild", (np.array([-2**31], np.int32), np.array([2**31 - 1], np.int32)))],
             2: [("path", links_of_sequences(2, paths=[[0, 1]])), ("reversed", links_of_sequences(2, paths=[[1, 0]])),
                 ("2-cycle", links_of_sequences(2, cycles=[[0, 1]])), ("unanswered", (np.array([-1, -1], np.int32), np.array([1, 0], np.int32)))],
             257: [("path over the workgroup edge", links_of_sequences(257, paths=[list(range(257))])),
                   ("only the link 255 > 256", links_of_sequences(257, paths=[[255, 256]]))],
             300: [("descending path", links_of_sequences(300, paths=[list(range(299, -1, -1))]))]}[n]
    for what, (idp, idn) in cases:
        if n == 0:
            assert_chains_equal(m.edge_chains(), np_chains(idp, idn), what)
            assert_polylines_equal(m.edge_polylines(), np_polylines(m.keylines(), ctx.p.fm), what)
            continue
        kl = upload_links(B, m, idp, idn)
        want = check_chains(m, kl, what)
        if what == "descending path":
            assert want[3] == 1 and list(want[1][:3]) == [299, 298, 297]
        assert_polylines_equal(m.edge_polylines(opts_of(B, DEFAULT_FILTER, 1), POSE), np_polylines(kl, ctx.p.fm, DEFAULT_FILTER, 1, POSE), what)
    ctx.close()


# ---- orderings and cycles ----------------------------------------------------------------------------------------------------------------
def test_orderings_and_cycles_at_1000(B):
    ctx = sized_ctx(B, 1000)
    m = sized_map(B, ctx, 1000)
    small = [[k, k + 1] for k in range(0, 200, 9)] + [[k + 2, k + 4, k + 3] for k in range(0, 200, 9)]
    beside = [list(range(k + 5, k + 9)) for k in range(0, 200, 9)] + [list(range(999, 300, -1))]
    idp_d, idn_d = (np.concatenate([a, np.full(988, -1, np.int32)]) for a in dirty_links())
    for what, (idp, idn) in (("one path in a random permutation: every round moves something", shuffled_path(1000, 4)),
                             ("one cycle over all 1000", links_of_sequences(1000, cycles=[list(range(1000))])),
                             ("one cycle in a random permutation", links_of_sequences(1000, cycles=[list(np.random.default_rng(6).permutation(1000))])),
                             ("cycles of 2 and 3 beside paths", links_of_sequences(1000, paths=beside, cycles=small)),
                             ("the dirty links", (idp_d, idn_d))):
        kl = upload_links(B, m, idp, idn)
        want = check_chains(m, kl, what)
        if "one cycle" in what:
            assert want[3] == 1 and (want[0]["flags"] == 1).all() and (want[0]["head"] == 0).all()
        if "2 and 3" in what:
            assert {2, 3} <= set(want[0]["length"][want[0]["flags"] == 1].tolist())
        assert_polylines_equal(m.edge_polylines(opts_of(B, DEFAULT_FILTER, 2)), np_polylines(kl, ctx.p.fm, DEFAULT_FILTER, 2), what)
    ctx.close()


def test_one_cycle_over_all_1024(B):
    """the size is the rounds' power of two: a span of exactly n"""
    ctx = sized_ctx(B, 1024)
    m = sized_map(B, ctx, 1024)
    for what, seq in (("in index order", list(range(1024))), ("shuffled", list(np.random.default_rng(8).permutation(1024)))):
        kl = upload_links(B, m, *links_of_sequences(1024, cycles=[seq]))
        want = check_chains(m, kl, what)
        assert want[3] == 1 and int(want[0]["length"][0]) == 1024
    ctx.close()


def test_the_full_envelope_of_65536_keylines(B):
    """keylines_max = 65 536 (16 rounds, 256 workgroups): one shuffled path over everything; one cycle of 65 535 beside a singleton"""
    frame = noise_frames(896, 640, 1, 3)[0]      # a noise frame of this size holds more candidates than the envelope
    ctx = B.Context(B.default_params(640, 896, fm=500.0, cx=447.5, cy=319.5, keylines_ref=60000, keylines_max=65536))
    m = ctx.detect_u8(frame, 0)
    n = m.size()
    assert n == 65536, n
    perm = np.random.default_rng(9).permutation(n)
    kl = upload_links(B, m, *links_of_sequences(n, paths=[list(perm)]))
    want = check_chains(m, kl, "shuffled path")
    assert want[3] == 1 and int(want[0]["head"][0]) == int(perm[0]) and int(want[0]["rank"][perm[-1]]) == n - 1
    rest = [int(k) for k in perm if k != 12345]
    kl = upload_links(B, m, *links_of_sequences(n, cycles=[rest]))
    want = check_chains(m, kl, "cycle of 65 535 beside a singleton")
    assert want[3] == 2 and sorted(np.diff(want[2]).tolist()) == [1, 65535]
    pts, refs2, lines, npts, nl = m.edge_polylines()
    assert (npts, nl) == (65535, 1) and tuple(lines[0]) == (0, 65535, 0, 1)
    cloud = m.point_cloud()
    assert pts[np.argsort(pts["keyline"], kind="stable")].tobytes() == cloud[cloud["keyline"] != 12345].tobytes()      # (the singleton is no line)
    ctx.close()


# ---- re-use, launches, resources ------------------------------------------------------------------------------------------------------------
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


def test_reuse_in_one_context_leaves_nothing_stale(B):
    """sizes 1000, then 3, then 0, then 1000 with other links: every call's result is its own map's"""
    ctx = sized_ctx(B, 1000)
    m_a, m_3, m_0, m_b = reuse_maps(B, ctx)
    kl_a = upload_links(B, m_a, *shuffled_path(1000, 1), seed=1)
    kl_3 = upload_links(B, m_3, *links_of_sequences(3, cycles=[[2, 0, 1]]), seed=2)
    kl_b = upload_links(B, m_b, *links_of_sequences(1000, cycles=[list(range(0, 1000, 2))], paths=[list(range(999, 0, -2))]), seed=3)
    for what, m, kl in (("1000", m_a, kl_a), ("3", m_3, kl_3), ("0", m_0, m_0.keylines()), ("1000 again", m_b, kl_b), ("3 again", m_3, kl_3)):
        check_chains(m, kl, what)
        assert_polylines_equal(m.edge_polylines(opts_of(B, DEFAULT_FILTER, 1), POSE), np_polylines(kl, ctx.p.fm, DEFAULT_FILTER, 1, POSE), what)
    ctx.close()


def test_the_entries_launch_what_the_header_documents_and_hold_one_allocation(B):
    """R + 5 launches for the chains and R + 8 for the polylines with R = ceil(log2(keylines_max)), the same at n = 0, 3 and 1000;
    one live resource more after the first call, none per call, none left after destroy"""
    live = B.test_live_resources()
    ctx = sized_ctx(B, 1000)
    m_a, m_3, m_0, m_b = reuse_maps(B, ctx)
    upload_links(B, m_a, *shuffled_path(1000, 1))
    for m in (m_a, m_3, m_0):
        m.keylines()
    R = rounds_of(1000)
    assert R == 10
    base = B.test_live_resources()
    want_c = {k: 1 for k in KERNELS_CHAINS}
    want_c["k_chain_round"] = R
    want_p = dict(want_c, **{k: 1 for k in KERNELS_POLY})
    ctx.profile(True)
    for m in (m_0, m_3, m_a):
        ctx.profile_reset()
        m.edge_chains()
        launches = {name: calls for name, (_, calls) in ctx.profile_read().items() if calls}
        assert launches == want_c and sum(launches.values()) == R + 5, (m.size(), launches)
        assert B.test_live_resources() == base + 1
        ctx.profile_reset()
        m.edge_polylines()
        launches = {name: calls for name, (_, calls) in ctx.profile_read().items() if calls}
        assert launches == want_p and sum(launches.values()) == R + 8, (m.size(), launches)
        assert B.test_live_resources() == base + 1
    ctx.profile(False)
    ctx.close()
    for m in (m_a, m_3, m_0, m_b):
        m.release()
    assert B.test_live_resources() == live


# ---- detected maps ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(160, 120), (320, 240)])
def test_detected_maps(B, size):
    """device detection, then the chains against the restatement of the downloaded keylines; polylines once the keylines have depths"""
    frames, cam = stream(size[0], size[1], 2)
    ctx = B.Context(params_for(B, cam))
    for k in range(2):
        m = ctx.detect_u8(frames[k], k * 50000)
        kl = m.keylines()
        want = check_chains(m, kl, (size, k))
        lengths = np.diff(want[2])
        print(size, "frame", k, "keylines", len(kl), "chains", want[3], "longest", int(lengths.max()), "cyclic", int((want[0]["flags"][want[0]["rank"] == 0]).sum()))
        assert len(kl) > 1000 and lengths.max() > 100
    rng = np.random.default_rng(7)
    kl["rho"] = rng.uniform(0.05, 3.0, len(kl)).astype(F32)
    kl["sigma_rho"] = (kl["rho"] * rng.uniform(0.0, 1.0, len(kl)).astype(F32)).astype(F32)
    kl["matches"] = rng.integers(0, 6, len(kl))
    m.upload(kl)
    for flt, min_len, pose in ((DEFAULT_FILTER, 8, None), (DEFAULT_FILTER, 8, POSE), (WIDE, 1, POSE), (DEFAULT_FILTER, 40, None)):
        want_p = np_polylines(kl, ctx.p.fm, flt, min_len, pose)
        assert len(want_p[0]) > 100 and len(want_p[2]) > 5
        assert_polylines_equal(m.edge_polylines(opts_of(B, flt, min_len), pose), want_p, (size, flt, min_len))
        assert_polylines_equal(B.edge_polylines_host(ctx.p.fm, kl, opts_of(B, flt, min_len), pose), want_p, (size, flt, min_len, "hook"))
    ctx.close()


# ---- polylines -------------------------------------------------------------------------------------------------------------------------
def test_polylines_planted_cases_caps_pose_and_the_clouds_bytes(B):
    """a chain cut into three lines by two planted filter failures, a chain below min_chain_length, a fully kept cycle (closed), cycles
    with one gap (no wrap); a cap below the counts; a pose; every point the bytes of its keyline's record in the map's cloud"""
    ctx = sized_ctx(B, 64)
    m = sized_map(B, ctx, 64)
    kl, want_lines = planted_polyline_map(B.KEYLINE_DTYPE)
    m.upload(kl)
    kl = m.keylines()
    for pose in (None, POSE):
        got = m.edge_polylines(None, pose)
        assert_polylines_equal(got, np_polylines(kl, ctx.p.fm, DEFAULT_FILTER, 8, pose), "planted")
        assert got[2].tobytes() == want_lines.tobytes()
        cloud = m.point_cloud(None, pose)
        rec_of = {int(k): j for j, k in enumerate(cloud["keyline"])}
        for p in got[0]:
            assert p.tobytes() == cloud[rec_of[int(p["keyline"])]].tobytes()
    full = m.edge_polylines(None, POSE)
    # caps below the counts: the counts stay, the leading records are the same, nothing is written behind the caps
    cp, cl, guard = 20, 5, 8
    pts = np.full((cp + guard) * 32, 0xA5, np.uint8)
    refs2 = np.full((cp + guard) * 8, 0xA5, np.uint8)
    lines = np.full((cl + guard) * 16, 0xA5, np.uint8)
    npts, nl = C.c_int(-1), C.c_int(-1)
    ip = C.POINTER(C.c_int)
    rc = B.lib().rebvio_hip_map_edge_polylines(m.h, None, B.cloud_pose(*POSE), pts.ctypes.data, refs2.ctypes.data_as(ip), cp, lines.ctypes.data, cl,
                                               C.byref(npts), C.byref(nl))
    assert rc == 0 and (npts.value, nl.value) == (55, 7)
    assert pts[:cp * 32].tobytes() == full[0][:cp].tobytes() and refs2[:cp * 8].tobytes() == full[1][:cp].tobytes()
    assert lines[:cl * 16].tobytes() == want_lines[:cl].tobytes()
    assert (pts[cp * 32:] == 0xA5).all() and (refs2[cp * 8:] == 0xA5).all() and (lines[cl * 16:] == 0xA5).all()
    assert B.lib().rebvio_hip_map_edge_polylines(m.h, None, None, None, None, 0, None, 0, C.byref(npts), C.byref(nl)) == 0
    assert (npts.value, nl.value) == (55, 7)
    # the chains' caps
    refs, order, starts, nk, nc = m.edge_chains(cap_keylines=10, cap_chains=2)
    want = np_chains(kl["id_prev"], kl["id_next"])
    assert (nk, nc, len(refs), len(starts)) == (64, 5, 10, 2)
    assert refs.tobytes() == want[0][:10].tobytes() and np.array_equal(order, want[1][:10]) and np.array_equal(starts, want[2][:2])
    assert B.lib().rebvio_hip_map_edge_chains(m.h, None, 0, None, None, 0, None, None) == 0      # every output may be NULL
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
    for call in (maps[1].edge_chains, maps[1].edge_polylines):
        with pytest.raises(B.HipError) as e:
            call()
        assert "error -7:" in str(e.value) and "R_prior_next" in str(e.value), str(e.value)
    check_chains(maps[0], maps[0].keylines(), "the pair's old map carries no promise")
    mid = ctx.track_pair_begin(maps[1], maps[2], R_prior=Rn)
    ctx.track_pair_finish_async(maps[1], maps[2], *vision_only_fusion(mid))
    ctx.track_pair_result()
    kl = maps[1].keylines()
    check_chains(maps[1], kl, "after the next begin")
    assert_polylines_equal(maps[1].edge_polylines(opts_of(B, WIDE, 8)), np_polylines(kl, ctx.p.fm, WIDE, 8), "after the next begin")
    L = B.lib()
    n, k = C.c_int(), C.c_int()
    assert L.rebvio_hip_map_edge_polylines(maps[1].h, B.default_polyline_opts(min_chain_length=0), None, None, None, 0, None, 0, C.byref(n), C.byref(k)) == -3
    assert L.rebvio_hip_map_edge_chains(maps[1].h, None, -1, None, None, 0, None, None) == -3
    ctx.close()
    assert L.rebvio_hip_map_edge_chains(maps[1].h, None, 0, None, None, 0, C.byref(n), C.byref(k)) == -10
    assert "destroyed" in L.rebvio_hip_last_error().decode()
    assert L.rebvio_hip_map_edge_polylines(maps[1].h, None, None, None, None, 0, None, 0, C.byref(n), C.byref(k)) == -10
    assert "destroyed" in L.rebvio_hip_last_error().decode()
    for m in maps:
        m.release()


# ---- with the tracker ----------------------------------------------------------------------------------------------------------------------
def test_calls_between_the_pairs_of_a_stream_disturb_nothing(B, small_stream):
    """12 frames: the pair records and the final keylines are equal word for word with and without both entries called between the pairs"""
    frames, cam = small_stream
    assert len(frames) == 12

    def run(with_chains):
        ctx = B.Context(params_for(B, cam, **KW_TRACK))
        maps = [ctx.detect_u8(frames[k], k * 50000) for k in range(12)]
        recs, seen = [], []
        for k in range(11):
            out = ctx.track_pair(maps[k], maps[k + 1])
            recs.append(rec(out, maps[k + 1].size()))
            if with_chains:
                refs, order, starts, nk, nc = maps[k + 1].edge_chains()
                pts, refs2, lines, npts, nl = maps[k + 1].edge_polylines()
                seen.append((nk, nc, npts, nl))
        final = maps[11].keylines()
        if with_chains:
            assert_polylines_equal(maps[11].edge_polylines(), np_polylines(final, ctx.p.fm), "the last map")
        ctx.close()
        return recs, final, seen

    plain, kl_plain, _ = run(False)
    chained, kl_chained, seen = run(True)
    print(seen)
    same_records(plain, chained, "with and without chain and polyline calls")
    assert kl_plain.tobytes() == kl_chained.tobytes()
    assert all(s[0] > 500 and s[1] > 10 for s in seen) and seen[-1][2] > 100 and seen[-1][3] > 3
