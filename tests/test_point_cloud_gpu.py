"""The point cloud of a map's depth-bearing keylines (rebvio_hip_map_point_cloud / _async) on the GPU.

The expected cloud is always np_cloud() of tests/support.py - a numpy fp32 restatement of the definition in include/rebvio_hip.h,
every operation one rounded fp32 operation in the header's order - applied to Map.keylines() downloaded immediately before the
extraction: the code under test never produces its own expectation. tests/test_point_cloud.py checks np_cloud() itself against
hand-computed cases."""
import ctypes as C

import numpy as np
import pytest

from conftest import params_for
from support import B, refusal_scene  # noqa: F401
from support import DEAD_MAP, assert_refused
from support import CLOUD_DTYPE, F32, KW_C2, enlarged_stream, np_cloud, np_passes, vision_only_fusion

pytestmark = pytest.mark.gpu

KW_SMALL = dict(keylines_ref=2000, keylines_max=3000)


def assert_cloud_equal(got, want, what):
    assert got.dtype == CLOUD_DTYPE, got.dtype
    assert len(got) == len(want), f"{what}: {len(got)} points, expected {len(want)}"
    for f in CLOUD_DTYPE.names:
        a, b = np.ascontiguousarray(got[f]).view(np.uint32), np.ascontiguousarray(want[f]).view(np.uint32)
        bad = np.flatnonzero((a != b).reshape(len(got), -1).any(axis=1))
        assert bad.size == 0, f"{what}: field {f} differs at {bad.size} points, first {bad[0]}: {got[f][bad[0]]} != {want[f][bad[0]]}"
    assert got.tobytes() == want.tobytes(), what


def flt_struct(B, flt):
    return B.CloudFilter(int(flt[0]), float(flt[1]), float(flt[2]), float(flt[3]))


def random_pose(seed):
    rng = np.random.default_rng(seed)
    w = rng.normal(size=3)
    w *= 1.1 / np.linalg.norm(w)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)  # Rodrigues
    return R.astype(F32), rng.normal(size=3).astype(F32), F32(0.37)


def crafted(kl, seed):
    """The map's keylines with random depth state: matches 0..5, rho over three decades, sigma_rho around half of rho."""
    rng = np.random.default_rng(seed)
    kl = kl.copy()
    n = len(kl)
    kl["matches"] = rng.integers(0, 6, n)
    kl["rho"] = np.exp(rng.uniform(np.log(2e-3), np.log(15.0), n)).astype(F32)
    kl["sigma_rho"] = (kl["rho"] * rng.uniform(0.0, 1.0, n).astype(F32)).astype(F32)
    return kl


# ---- 1: a tracked map ---------------------------------------------------------------------------------------------------
def test_cloud_of_a_tracked_map_is_bit_exact(B, c2_stream):
    """Seven pairs of the 640x480 stream through track_pair, then the newest map's cloud for the identity pose and for a random
    rotation, translation and scale: records, count and order bit-identical to np_cloud(). The thresholds come from the
    downloaded keylines (max_rel_sigma = median of sigma_rho / rho among keylines with matches >= 2), so the selection is neither
    empty nor everything: its share of the map must lie in 0.2 .. 0.8 and exceed 1000 points."""
    frames, cam = c2_stream
    ctx = B.Context(params_for(B, cam, **KW_C2))
    maps = [ctx.detect_u8(frames[i], i * 50000) for i in range(len(frames))]
    assert len(maps) >= 7
    for k in range(len(maps) - 1):
        assert ctx.track_pair(maps[k], maps[k + 1]).status == 0
    m = maps[-1]
    kl = m.keylines()
    seen = kl["matches"] >= 2
    rel = (kl["sigma_rho"][seen] / kl["rho"][seen]).astype(F32)
    flt = (2, F32(np.median(rel)), 1e-3, 20.0)
    default_share = np_passes(kl, 2, 0.5, 1e-3, 20.0).mean()
    for pose, what in ((None, "identity pose"), (random_pose(5), "random pose")):
        want = np_cloud(kl, ctx.p.fm, flt, pose)
        got, count = m.point_cloud(flt_struct(B, flt), pose, return_count=True)
        share = len(want) / len(kl)
        print(f"{what}: map {len(kl)} keylines, matches >= 2: {seen.sum()}, max_rel_sigma {flt[1]:.4f}, cloud {len(want)} "
              f"({share:.3f} of the map); default filter passes {default_share:.3f}")
        assert count == len(want)
        assert_cloud_equal(got, want, what)
        assert np.all(np.diff(got["keyline"]) > 0)
        assert 0.2 <= share <= 0.8 and len(want) > 1000, (share, len(want))
    # the default filter and pose (NULL, NULL) are what rebvio_hip_default_cloud_filter says
    d = B.default_cloud_filter()
    assert_cloud_equal(m.point_cloud(), np_cloud(kl, ctx.p.fm, (d.min_matches, d.max_rel_sigma, d.rho_min, d.rho_max)), "defaults")
    ctx.close()


# ---- 2: every filter term alone, at its boundary ------------------------------------------------------------------------
def test_each_filter_term_at_its_boundary(B, small_stream):
    frames, cam = small_stream
    ctx = B.Context(params_for(B, cam, **KW_SMALL))
    m = ctx.detect_u8(frames[0], 0)
    kl = m.keylines()
    assert len(kl) > 45
    flt = (3, F32(0.25), F32(0.1), F32(4.0))
    up, dn = F32(np.inf), F32(-np.inf)
    kl["matches"], kl["rho"], kl["sigma_rho"] = 0, F32(1.0), F32(0.1)   # everything else fails on matches alone
    rho_odd = F32(0.7)
    edge = F32(flt[1] * rho_odd)                                          # max_rel_sigma * rho, rounded once
    cases = [  # (matches, rho, sigma_rho, passes)
        (3, 1.0, 0.1, True), (2, 1.0, 0.1, False), (4, 1.0, 0.1, True),                      # min_matches (inclusive)
        (3, flt[2], 0.0, True), (3, np.nextafter(flt[2], dn), 0.0, False),                  # rho_min (inclusive)
        (3, flt[3], 0.1, True), (3, np.nextafter(flt[3], up), 0.1, False),                  # rho_max (inclusive)
        (3, rho_odd, edge, True), (3, rho_odd, np.nextafter(edge, up), False),              # max_rel_sigma * rho (inclusive)
        (3, 0.0, 0.0, False), (3, -1.0, 0.0, False), (3, -1.0, -1.0, False),                # rho = 0, negative rho
        (3, np.nan, 0.1, False), (3, np.inf, 0.1, False), (3, 1.0, np.nan, False), (3, 1.0, np.inf, False),
        (3, np.nan, np.nan, False), (3, 1.0, -0.5, True),
    ]
    at = 7 + 2 * np.arange(len(cases))  # spread, not adjacent
    for i, (mt, rho, sig, _) in zip(at, cases):
        kl["matches"][i], kl["rho"][i], kl["sigma_rho"][i] = mt, F32(rho), F32(sig)
    m.upload(kl)
    kl2 = m.keylines()
    assert kl2.tobytes() == kl.tobytes()
    got = m.point_cloud(flt_struct(B, flt))
    expected = [int(i) for i, c in zip(at, cases) if c[3]]
    assert got["keyline"].tolist() == expected, (got["keyline"].tolist(), expected)
    assert_cloud_equal(got, np_cloud(kl2, ctx.p.fm, flt), "boundary cases")
    assert np.isfinite(got["xyz"]).all()
    ctx.close()


# ---- 3: cap ---------------------------------------------------------------------------------------------------------
def test_cap_below_count_writes_the_first_cap_points_only(B, small_stream):
    frames, cam = small_stream
    ctx = B.Context(params_for(B, cam, **KW_SMALL))
    m = ctx.detect_u8(frames[1], 0)
    kl = crafted(m.keylines(), 3)
    m.upload(kl)
    flt = (2, 0.6, 1e-3, 20.0)
    full, count = m.point_cloud(flt_struct(B, flt), return_count=True)
    assert count == len(full) > 50
    assert_cloud_equal(full, np_cloud(kl, ctx.p.fm, flt), "full cloud")
    cap, guard = count // 3, 16
    buf = np.full((cap + guard) * 32, 0xA5, np.uint8)
    n = C.c_int(-1)
    rc = B.lib().rebvio_hip_map_point_cloud(m.h, flt_struct(B, flt), None, buf.ctypes.data, cap, C.byref(n))
    assert rc == 0 and n.value == count
    assert buf[:cap * 32].tobytes() == full[:cap].tobytes()
    assert (buf[cap * 32:] == 0xA5).all(), "records written beyond cap"
    n = C.c_int(-1)
    assert B.lib().rebvio_hip_map_point_cloud(m.h, flt_struct(B, flt), None, None, 0, C.byref(n)) == 0
    assert n.value == count
    ctx.close()


# ---- 4: sizes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmax", [50, 150, 1000])
def test_small_and_odd_map_sizes(B, small_stream, kmax):
    """A map of fewer than 64 keylines, maps whose size is no multiple of 64 or 256, and an empty selection."""
    frames, cam = small_stream
    ctx = B.Context(params_for(B, cam, keylines_ref=max(kmax - 10, 10), keylines_max=kmax))
    m = ctx.detect_u8(frames[2], 0)
    n = m.size()
    print("keylines_max", kmax, "map size", n)
    assert 0 < n <= kmax and n % 64 != 0
    if kmax == 50:
        assert n < 64
    kl = crafted(m.keylines(), kmax)
    m.upload(kl)
    flt = (1, 0.5, 1e-2, 10.0)
    want = np_cloud(kl, ctx.p.fm, flt, random_pose(kmax))
    assert 0 < len(want) < n
    assert_cloud_equal(m.point_cloud(flt_struct(B, flt), random_pose(kmax)), want, f"{n} keylines")
    none, count = m.point_cloud(flt_struct(B, (10 ** 9, 0.5, 1e-2, 10.0)), return_count=True)
    assert count == 0 and len(none) == 0
    q = ctx.point_cloud_async(m, flt_struct(B, (10 ** 9, 0.5, 1e-2, 10.0)))
    assert len(q.wait()) == 0
    q.release()
    ctx.close()


def test_a_map_that_fills_the_keyline_envelope(B):
    """keylines_max = 65 536 on a 2304 x 1900 frame with keylines_ref 60 000: a map of more than 32 768 keylines, i.e. more than
    128 workgroups' counts in the block-offset pass, through both entries."""
    W, H = 2304, 1900
    frames, cam = enlarged_stream(W, H, 3)
    ctx = B.Context(B.default_params(H, W, fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=60000, keylines_max=65536))
    maps = [ctx.detect_u8(frames[i], i * 50000) for i in range(3)]
    m = max(maps, key=lambda x: x.size())
    n = m.size()
    print("map size", n)
    assert n > 32768
    kl = crafted(m.keylines(), 11)
    m.upload(kl)
    flt = (2, 0.5, 1e-2, 10.0)
    pose = random_pose(2)
    want = np_cloud(kl, ctx.p.fm, flt, pose)
    assert len(want) > 8000
    assert_cloud_equal(m.point_cloud(flt_struct(B, flt), pose), want, "synchronous")
    q = ctx.point_cloud_async(m, flt_struct(B, flt), pose)
    assert_cloud_equal(q.wait(), want, "queued")
    assert q.device_points
    q.release()
    everything = (0, F32(np.inf), 1e-30, F32(np.inf))
    assert_cloud_equal(m.point_cloud(flt_struct(B, everything)), np_cloud(kl, ctx.p.fm, everything), "every keyline")
    ctx.close()


# ---- 5: the queued entry ---------------------------------------------------------------------------------------------
def _run_halves(B, frames, cam, pairs, clouds, flt, pose, sync_last=False):
    """begin(k), result(k-1), finish_async(k) over `pairs` pairs as rebvio::Rebvio orders them; clouds: point_cloud_async on the new
    map between every finish_async(k) and begin(k+1). Returns (PairMid bytes, result tuples, keylines of every map, clouds)."""
    ctx = B.Context(params_for(B, cam, **KW_C2))
    maps = [ctx.detect_u8(frames[i], i * 50000) for i in range(pairs + 1)]
    mids, results, queued = [], [], []
    for k in range(pairs):
        mid = ctx.track_pair_begin(maps[k], maps[k + 1])
        if k > 0:
            results.append(ctx.track_pair_result())
        mids.append(bytes(mid))
        ctx.track_pair_finish_async(maps[k], maps[k + 1], *vision_only_fusion(mid))
        if clouds:
            queued.append(ctx.point_cloud_async(maps[k + 1], flt_struct(B, flt), pose))
    results.append(ctx.track_pair_result())
    out_clouds = []
    for q in queued:
        out_clouds.append(q.wait())
        q.release()
    last = maps[-1].point_cloud(flt_struct(B, flt), pose) if sync_last else None
    kls = [m.keylines().tobytes() for m in maps]
    ctx.close()
    return mids, results, kls, out_clouds, last


def test_queued_cloud_equals_the_synchronous_one_and_moves_nothing_else(B, c2_stream):
    """Run A: six pairs in halves without a cloud call. Run B: the same with a cloud queued between every finish_async(k) and
    begin(k+1): every PairMid, result tuple and final keyline of B bit-identical to A, and the cloud queued after pair k equal to
    the synchronous cloud of a run stopped after pair k."""
    frames, cam = c2_stream
    flt, pose = (1, 1.0, 1e-3, 20.0), random_pose(9)
    mids_a, res_a, kl_a, _, _ = _run_halves(B, frames, cam, 6, False, flt, pose)
    mids_b, res_b, kl_b, clouds, _ = _run_halves(B, frames, cam, 6, True, flt, pose)
    assert mids_a == mids_b, [i for i in range(6) if mids_a[i] != mids_b[i]]
    assert res_a == res_b, (res_a, res_b)
    assert all(r[3] == 0 for r in res_a), res_a
    assert kl_a == kl_b, [i for i in range(7) if kl_a[i] != kl_b[i]]
    assert len(clouds) == 6
    for k in range(6):
        _, _, _, _, sync = _run_halves(B, frames, cam, k + 1, False, flt, pose, sync_last=True)
        print("pair", k, "queued cloud", len(clouds[k]), "synchronous", len(sync))
        assert_cloud_equal(clouds[k], sync, f"cloud queued after pair {k}")
    assert len(clouds[-1]) > 1000


# ---- 6: the promise ---------------------------------------------------------------------------------------------------
def test_a_map_rotated_for_the_next_pair_is_refused_until_that_pair_begins(B, c2_stream):
    frames, cam = c2_stream
    ctx = B.Context(params_for(B, cam, **KW_C2))
    maps = [ctx.detect_u8(frames[i], i * 50000) for i in range(3)]
    c, s = F32(np.cos(0.01)), F32(np.sin(0.01))
    Rn = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], F32)
    mid = ctx.track_pair_begin(maps[0], maps[1])
    ctx.track_pair_finish_async(maps[0], maps[1], *vision_only_fusion(mid), R_prior_next=Rn)
    assert ctx.track_pair_result()[3] == 0
    for call in (lambda: maps[1].point_cloud(cap=0), lambda: ctx.point_cloud_async(maps[1])):
        with pytest.raises(B.HipError) as e:
            call()
        assert "error -7:" in str(e.value) and "R_prior_next" in str(e.value), str(e.value)
    maps[0].point_cloud()   # the pair's old map carries no promise
    mid = ctx.track_pair_begin(maps[1], maps[2], R_prior=Rn)
    ctx.track_pair_finish_async(maps[1], maps[2], *vision_only_fusion(mid))
    assert ctx.track_pair_result()[3] == 0
    kl = maps[1].keylines()
    flt = (1, 1.0, 1e-3, 20.0)
    want = np_cloud(kl, ctx.p.fm, flt)
    assert_cloud_equal(maps[1].point_cloud(flt_struct(B, flt)), want, "after the next begin, synchronous")
    q = ctx.point_cloud_async(maps[1], flt_struct(B, flt))
    assert_cloud_equal(q.wait(), want, "after the next begin, queued")
    q.release()
    ctx.close()


# ---- 7: refusals ------------------------------------------------------------------------------------------------------
def test_refusals(B, small_stream):
    frames, cam = small_stream
    ctx = B.Context(params_for(B, cam, **KW_SMALL))
    m = ctx.detect_u8(frames[0], 0)
    L = B.lib()
    n = C.c_int()
    nan = float("nan")
    for flt, text in (((2, 0.5, 0.0, 20.0), "rho_min must be > 0"), ((2, 0.5, -1.0, 20.0), "rho_min must be > 0"),
                      ((2, 0.5, 5.0, 4.0), "rho_min > rho_max"), ((2, -0.1, 1e-3, 20.0), "max_rel_sigma must be >= 0"),
                      ((2, nan, 1e-3, 20.0), "NaN"), ((2, 0.5, nan, 20.0), "NaN"), ((2, 0.5, 1e-3, nan), "NaN")):
        assert L.rebvio_hip_map_point_cloud(m.h, flt_struct(B, flt), None, None, 0, C.byref(n)) == -3, flt
        assert text in L.rebvio_hip_last_error().decode(), (flt, L.rebvio_hip_last_error().decode())
        h = C.c_void_p()
        assert L.rebvio_hip_map_point_cloud_async(ctx.h, m.h, flt_struct(B, flt), None, C.byref(h)) == -3, flt
        assert text in L.rebvio_hip_last_error().decode() and not h.value
    assert L.rebvio_hip_map_point_cloud(None, None, None, None, 0, C.byref(n)) == -3
    assert "null map" in L.rebvio_hip_last_error().decode()
    h = C.c_void_p()
    assert L.rebvio_hip_map_point_cloud_async(ctx.h, None, None, None, C.byref(h)) == -3
    assert "null" in L.rebvio_hip_last_error().decode()
    assert L.rebvio_hip_map_point_cloud(m.h, None, None, None, 5, C.byref(n)) == -3   # five records, nowhere to put them
    assert "points buffer" in L.rebvio_hip_last_error().decode()
    q = ctx.point_cloud_async(m)
    ctx.close()
    assert L.rebvio_hip_map_point_cloud(m.h, None, None, None, 0, C.byref(n)) == -10
    assert "destroyed" in L.rebvio_hip_last_error().decode()
    with pytest.raises(B.HipError) as e:
        q.wait()
    assert "error -10:" in str(e.value) and "destroyed" in str(e.value)
    q.release()
    m.release()


# ---- the refusal table: every shared refusal with its code and whole text; which one wins when several apply ------
REFUSED = {
    "queued: map of another context": (lambda s: s.other.point_cloud_async(s.m), -3, "map_point_cloud_async: map of another context"),
    "queued: wins: a destroyed map over another context": (lambda s: s.other.point_cloud_async(s.dm), -10, DEAD_MAP),
    "queued: wins: the filter over another context": (lambda s: s.other.point_cloud_async(s.m, s.B.default_cloud_filter(rho_min=-1.0)), -3,
                                                      "map_point_cloud_async: filter rho_min must be > 0"),
}
@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusal_table(refusal_scene, case):
    """every refusal of the table with its return code and its whole rebvio_hip_last_error text; nothing is allocated"""
    assert_refused(refusal_scene, *REFUSED[case])
