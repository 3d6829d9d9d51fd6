"""The point cloud of a keyframe snapshot on the device: rebvio_hip_kf_snapshot_point_cloud / _async (k_kf_cloud_count,
k_kf_cloud_emit, then k_cloud_copy). The expected cloud is always support.np_cloud applied to the snapshot's download from just
before (tests/kf_cloud_ref.py), and the host hook's (rebvio_hip_test_kf_cloud_host) next to it: device = hook = np_cloud bit for
bit - the definition has no sum and every operation is one rounded fp32 operation, so equality is the bound.

A snapshot's content is planted by uploading keylines into a map of exactly that size and snapshotting it, the way
tests/test_keyframe_fuse_gpu.py builds its own. All contexts are 160x120 with keylines_max <= 800 unless a case says otherwise."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import params_for
from kf_align_ref import GUARD, craft_against, craft_kf_keylines, unit_of
from kf_cloud_ref import DEFAULT, ODD, SIZES, assert_cloud_equal, edge_rows, flt_dict, np_kf_cloud, random_pose, random_snapshot
from kf_fuse_ref import np_kf_fuse, perturbed
from kf_pose_ref import true_motion
from support import B, refusal_scene  # noqa: F401
from support import DEAD_SNAPSHOT, assert_refused, assert_release_keeps_the_message
from support import F32, TS, enlarged_stream, np_passes, vision_only_fusion

pytestmark = pytest.mark.gpu

W, H, NF = 160, 120, 10
KW_STREAM = dict(keylines_ref=600, keylines_max=800, global_min_matches_threshold=50)      # the stream of the pose tests: every pair tracks


@functools.lru_cache(maxsize=None)
def stream():
    from rebvio_amd import synth
    return synth.render_stream(W, H, NF)


def sized_maps(B, n, count=1):
    """(context, maps) with exactly n keylines each: keylines_max = n truncates the frames' keylines (n = 0: blank frames)"""
    frames, cam = stream()
    if n == 0:
        ctx = B.Context(params_for(B, cam, **KW_STREAM))
        maps = [ctx.detect_u8(np.full((H, W), 128, np.uint8), k * TS) for k in range(count)]
    else:
        ctx = B.Context(params_for(B, cam, keylines_ref=max(1, n - 1), keylines_max=n, global_min_matches_threshold=1))
        maps = [ctx.detect_u8(frames[1 + k], k * TS) for k in range(count)]
    assert all(m.size() == n for m in maps), (n, [m.size() for m in maps])
    return ctx, maps


def planted(m, prs4, mt):
    """a snapshot holding exactly (prs4, mt): uploaded into the map m, snapshotted, downloaded and compared"""
    kl = m.keylines()
    assert len(kl) == len(prs4)
    if len(kl):
        kl["pos_img"], kl["rho"], kl["sigma_rho"], kl["matches"] = prs4[:, :2], prs4[:, 2], prs4[:, 3], mt
        m.upload(kl)
    snap = m.keyframe_snapshot()
    p, q = snap.download()
    assert p.tobytes() == np.asarray(prs4, F32).tobytes() and q.tobytes() == np.asarray(mt, np.uint32).tobytes()
    return snap


def all_three(B, ctx, snap, flt, pose, what):
    """device = hook = np_cloud(download()), with the count; returns the cloud"""
    prs4, mt = snap.download()
    want = np_kf_cloud(prs4, mt, ctx.p.fm, flt, pose)
    hook, hc = B.kf_cloud_host(ctx.p.fm, prs4, mt, flt_dict(flt), pose, return_count=True)
    got, count = snap.point_cloud(flt_dict(flt), pose, return_count=True)
    assert count == hc == len(want), (what, count, hc, len(want))
    assert_cloud_equal(hook, want, what + ": hook")
    assert_cloud_equal(got, want, what + ": device")
    assert np.all(np.diff(got["keyline"]) > 0)
    return got


def device_bytes(addr, nbytes):
    """nbytes of device memory at addr, read with the HIP runtime the library itself is linked to"""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.zeros(nbytes, np.uint8)
    assert hip.hipMemcpy(out.ctypes.data, addr, nbytes, 2) == 0      # hipMemcpyDeviceToHost
    return out


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES + (800,))
def test_device_equals_hook_equals_np_cloud(B, n):
    """the wave edge, the workgroup edge, a partly filled last workgroup; identity and random poses, two filters"""
    ctx, (m,) = sized_maps(B, n)
    for flt in (DEFAULT, ODD):
        prs4, mt = random_snapshot(n, 300 + n, flt)
        snap = planted(m, prs4, mt)
        for pose, what in ((None, "identity"), (random_pose(n + 1), "random pose")):
            got = all_three(B, ctx, snap, flt, pose, f"n {n}, {what}")
            assert n < 64 or 0 < len(got) < n
        snap.release()
    ctx.close()


def test_an_empty_workgroup_in_front_of_a_filled_one(B):
    ctx, (m,) = sized_maps(B, 800)
    prs4, mt = random_snapshot(800, 5)
    mt[:256] = 0                                     # workgroup 0 passes nothing
    mt[512:768] = 0                                  # nor does workgroup 2
    snap = planted(m, prs4, mt)
    got = all_three(B, ctx, snap, DEFAULT, random_pose(3), "empty workgroups")
    assert len(got) > 100 and got["keyline"].min() >= 256 and ((got["keyline"] >= 768) | (got["keyline"] < 512)).all()
    snap.release()
    ctx.close()


def test_a_snapshot_that_fills_the_keyline_envelope(B):
    """65 536 keylines on a 2304 x 1900 frame, more than 32 768 of them passing: all 256 block counts are in play and the offsets
    lie above 2^15; through both entries"""
    Wb, Hb = 2304, 1900
    frames, cam = enlarged_stream(Wb, Hb, 3)
    ctx = B.Context(B.default_params(Hb, Wb, fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=60000, keylines_max=65536))
    m = max((ctx.detect_u8(frames[i], i * 50000) for i in range(3)), key=lambda x: x.size())
    assert m.size() == 65536
    flt = (0, F32(0.5), F32(1e-3), F32(20.0))         # (any matches: about 0.6 of random_snapshot's draws pass)
    prs4, mt = random_snapshot(65536, 11, flt)
    snap = planted(m, prs4, mt)
    pose = random_pose(2)
    got = all_three(B, ctx, snap, flt, pose, "large")
    print("large: cloud of", len(got))
    assert len(got) > 32768 and got["keyline"][-1] > 65536 - 256 and got["keyline"][0] < 256
    q = snap.point_cloud_async(flt_dict(flt), pose)
    assert q.wait().tobytes() == got.tobytes()
    q.release()
    snap.release()
    ctx.close()


# ---- 2. the filter ----------------------------------------------------------------------------------------------------------------
def test_filter_terms_on_and_off_their_bounds_and_non_finite_values(B):
    ctx, (m,) = sized_maps(B, 257)
    for flt in (DEFAULT, ODD):
        rows = edge_rows(flt)
        prs4 = np.zeros((257, 4), F32)
        prs4[:, 2], prs4[:, 3] = 1.0, 0.01
        mt = np.zeros(257, np.uint32)                # everything else fails on matches (min_matches >= 2 in both filters)
        at = 3 + 16 * np.arange(len(rows))           # spread over the waves and both workgroups
        assert at[-1] < 257
        for i, r in zip(at, rows):
            prs4[i], mt[i] = r[:4], r[4]
        snap = planted(m, prs4, mt)
        got = all_three(B, ctx, snap, flt, None, f"edges {flt}")
        assert got["keyline"].tolist() == [int(i) for i, r in zip(at, rows) if r[5]]
        assert np.isfinite(got["xyz"]).all() and (got["rho"] > 0).all()
        assert not got["gradient_norm"].view(np.uint32).any()
        # a filter that selects nothing
        none, count = snap.point_cloud(dict(min_matches=0xFFFFFFFF, rho_min=19.0, rho_max=19.5), return_count=True)
        assert count == 0 and len(none) == 0
        q = snap.point_cloud_async(dict(min_matches=0xFFFFFFFF, rho_min=19.0, rho_max=19.5))
        assert len(q.wait()) == 0
        q.release()
        snap.release()
    ctx.close()


# ---- 3. cap -----------------------------------------------------------------------------------------------------------------------
def test_cap_below_count_and_cap_zero(B):
    ctx, (m,) = sized_maps(B, 800)
    snap = planted(m, *random_snapshot(800, 9))
    full, count = snap.point_cloud(return_count=True)
    assert count == len(full) > 200
    cap, guard = count // 3, 16
    buf = np.full((cap + guard) * 32, 0xA5, np.uint8)
    n = C.c_int(-1)
    L = B.lib()
    assert L.rebvio_hip_kf_snapshot_point_cloud(snap.h, None, None, buf.ctypes.data, cap, C.byref(n)) == 0 and n.value == count
    assert buf[:cap * 32].tobytes() == full[:cap].tobytes()
    assert (buf[cap * 32:] == 0xA5).all(), "records written beyond cap"
    n = C.c_int(-1)
    assert L.rebvio_hip_kf_snapshot_point_cloud(snap.h, None, None, None, 0, C.byref(n)) == 0 and n.value == count
    more, c2 = snap.point_cloud(cap=count + 100, return_count=True)             # (a cap above keylines_max is the buffer's capacity)
    assert c2 == count and more.tobytes() == full.tobytes()
    snap.release()
    ctx.close()


# ---- 4. after a fusion -----------------------------------------------------------------------------------------------------------
def test_the_cloud_shows_the_fused_depths(B):
    """the cloud after one and after two fuse_depth calls = np_cloud of the downloaded, fused snapshot; with max_rel_sigma at the
    median sigma_rho / rho of the unfused keylines (the filter of tests/test_keyframe_cloud.py's purpose test) it differs from the
    cloud taken before"""
    ctx, (mk, mc) = sized_maps(B, 800, 2)
    kl = mc.keylines()
    ids, dists = mc.distance_field()
    cam = (ctx.p.fm, ctx.p.cx, ctx.p.cy, ctx.rows, ctx.cols)
    A = dict(craft_against(kl, ids.reshape(-1), dists.reshape(-1), 1, cam))
    A["prs4"], _ = perturbed(A, 101)
    base = mk.keylines()
    base["matches"] = 0
    mk.upload(craft_kf_keylines(base, A, min(len(A["prs4"]), len(base))))
    snap = mk.keyframe_snapshot()
    snap.add_normals(mk)
    R, t = true_motion()
    prs4, mt = snap.download()
    ref = np_kf_fuse(cam, prs4, mt, snap.normals(), np.ascontiguousarray(kl["pos"]), unit_of(kl), ids.reshape(-1), dists.reshape(-1), R, t)
    assert min(ref["guards"].values()) > GUARD
    k = np.zeros(len(prs4), np.dtype([("rho", "<f4"), ("sigma_rho", "<f4"), ("matches", "<u4")]))
    k["rho"], k["sigma_rho"], k["matches"] = prs4[:, 2], prs4[:, 3], mt
    ok = np_passes(k, *DEFAULT)
    tight = (2, F32(np.median((prs4[ok, 3] / prs4[ok, 2]).astype(F32))), F32(1e-3), F32(20.0))
    pose = random_pose(4)
    clouds = [all_three(B, ctx, snap, tight, pose, "before")]
    for call in (1, 2):
        out = snap.fuse_depth(mc, R, t)
        assert out.fused > 100, call
        if call == 1:
            assert snap.download()[0].tobytes() == ref["prs4"].tobytes()
        clouds.append(all_three(B, ctx, snap, tight, pose, f"after fusion {call}"))
        all_three(B, ctx, snap, DEFAULT, pose, f"after fusion {call}, default filter")
        assert clouds[-1].tobytes() != clouds[-2].tobytes()
    print("tight filter: points before, after one, after two fusions:", [len(c) for c in clouds])
    snap.release()
    ctx.close()


# ---- 5. the queued form ------------------------------------------------------------------------------------------------------------
def test_queued_form_equals_the_synchronous_one_and_device_points_hold_the_records(B):
    ctx, (m,) = sized_maps(B, 800)
    snap = planted(m, *random_snapshot(800, 13, ODD))
    pose = random_pose(6)
    sync = snap.point_cloud(flt_dict(ODD), pose)
    q = snap.point_cloud_async(flt_dict(ODD), pose)
    got = q.wait()
    assert_cloud_equal(got, sync, "queued")
    assert len(got) > 100 and q.device_points
    dev = device_bytes(q.device_points, len(got) * 32)
    assert dev.tobytes() == got.tobytes()
    view = q.wait(copy=False)
    assert view.tobytes() == got.tobytes()
    q.release()
    snap.release()
    ctx.close()


def test_a_handle_released_without_a_wait_and_reused(B):
    ctx, (m,) = sized_maps(B, 800)
    snap = planted(m, *random_snapshot(800, 17))
    first = snap.point_cloud_async()
    first.wait()
    buf = first.device_points
    first.release()
    live = B.test_live_resources()
    for k in range(4):
        snap.point_cloud_async(None, random_pose(k)).release()       # never waited for
    pose = random_pose(40)
    q = snap.point_cloud_async(None, pose)
    got = q.wait()
    prs4, mt = snap.download()
    assert_cloud_equal(got, np_kf_cloud(prs4, mt, ctx.p.fm, DEFAULT, pose), "after four unwaited extractions")
    assert q.device_points == buf and B.test_live_resources() == live     # the one pooled buffer all along
    q.release()
    snap.release()
    ctx.close()


def _run_halves(B, pairs, clouds):
    """begin(k), result(k-1), finish_async(k) over `pairs` pairs; clouds: the snapshot of map 1 is taken behind pair 0 and its cloud
    queued between every finish_async(k) and begin(k+1). Returns (PairMid bytes, result tuples, keylines of every map, clouds, the
    expected cloud)."""
    frames, cam = stream()
    ctx = B.Context(params_for(B, cam, **KW_STREAM))
    maps = [ctx.detect_u8(frames[i], i * TS) for i in range(pairs + 1)]
    mids, results, queued, snap = [], [], [], None
    pose = random_pose(8)
    for k in range(pairs):
        mid = ctx.track_pair_begin(maps[k], maps[k + 1])
        if k > 0:
            results.append(ctx.track_pair_result())
        mids.append(bytes(mid))
        ctx.track_pair_finish_async(maps[k], maps[k + 1], *vision_only_fusion(mid))
        if clouds:
            if snap is None:
                snap = maps[1].keyframe_snapshot()
            queued.append(snap.point_cloud_async(dict(min_matches=1, max_rel_sigma=1.0), pose))
    results.append(ctx.track_pair_result())
    out = []
    for q in queued:
        out.append(q.wait())
        q.release()
    want = None
    if snap is not None:
        prs4, mt = snap.download()
        want = np_kf_cloud(prs4, mt, ctx.p.fm, (1, F32(1.0), F32(1e-3), F32(20.0)), pose)
        snap.release()
    kls = [m.keylines().tobytes() for m in maps]
    ctx.close()
    return mids, results, kls, out, want


def test_clouds_queued_between_the_halves_move_nothing_else(B):
    mids_a, res_a, kl_a, _, _ = _run_halves(B, 6, False)
    mids_b, res_b, kl_b, clouds, want = _run_halves(B, 6, True)
    assert mids_a == mids_b, [i for i in range(6) if mids_a[i] != mids_b[i]]
    assert res_a == res_b, (res_a, res_b)
    assert all(r[3] == 0 for r in res_a), res_a
    assert kl_a == kl_b, [i for i in range(7) if kl_a[i] != kl_b[i]]
    assert len(clouds) == 6 and len(want) > 50
    for k, c in enumerate(clouds):
        assert_cloud_equal(c, want, f"cloud queued behind pair {k}")


# ---- 6. determinism and accounting -------------------------------------------------------------------------------------------------
def test_two_extractions_are_byte_identical_and_launch_what_is_documented(B):
    ctx, (m,) = sized_maps(B, 800)
    snap = planted(m, *random_snapshot(800, 21))
    pose = random_pose(1)
    a = snap.point_cloud(None, pose)
    ctx.profile_reset()
    ctx.profile(True)
    b = snap.point_cloud(None, pose)
    launches = {name: calls for name, (_, calls) in ctx.profile_read().items() if calls}
    assert launches == dict(k_kf_cloud_count=1, k_kf_cloud_emit=1, k_cloud_copy=1), launches     # two on the track stream, one on the cloud stream
    q = snap.point_cloud_async(None, pose)
    c = q.wait()
    q.release()
    launches = {name: calls for name, (_, calls) in ctx.profile_read().items() if calls}
    ctx.profile(False)
    assert launches == dict(k_kf_cloud_count=2, k_kf_cloud_emit=2, k_cloud_copy=2), launches
    assert a.tobytes() == b.tobytes() == c.tobytes() and len(a) > 200
    snap.release()
    ctx.close()


def test_resources_are_the_context_cloud_pool(B):
    start = B.test_live_resources()
    ctx, (m,) = sized_maps(B, 65)
    snap = planted(m, *random_snapshot(65, 2))
    base = B.test_live_resources()
    q1 = ctx.point_cloud_async(m)                    # the context's first cloud, a map's: scratch, stream, one pooled buffer
    first_map = B.test_live_resources() - base
    q2 = snap.point_cloud_async()                    # none is free: one more pooled buffer, nothing else
    one_buffer = B.test_live_resources() - base - first_map
    q3 = ctx.point_cloud_async(m)                    # what a map's cloud adds in the same place
    assert B.test_live_resources() - base - first_map == 2 * one_buffer and first_map == one_buffer + 2 and one_buffer > 0
    for q in (q1, q2, q3):
        q.wait()
        q.release()
    held = B.test_live_resources()
    snap.point_cloud()
    snap.point_cloud_async().release()
    assert B.test_live_resources() == held           # buffers are free: nothing is added
    snap.release()
    m.release()
    ctx.close()
    assert B.test_live_resources() == start
    # a fresh context whose first cloud is a snapshot's: it makes what a map's first cloud makes, and the map's then adds nothing
    ctx, (m,) = sized_maps(B, 65)
    snap = planted(m, *random_snapshot(65, 2))
    base = B.test_live_resources()
    snap.point_cloud()
    assert B.test_live_resources() - base == first_map
    m.point_cloud()
    assert B.test_live_resources() - base == first_map
    snap.release()
    m.release()
    ctx.close()
    assert B.test_live_resources() == start


# ---- 7. errors and lifetime ---------------------------------------------------------------------------------------------------------
def test_refusals_and_a_destroyed_context(B):
    ctx, (m,) = sized_maps(B, 65)
    snap = planted(m, *random_snapshot(65, 3))
    L = B.lib()
    err = lambda: L.rebvio_hip_last_error().decode()
    n, h = C.c_int(), C.c_void_p()
    sync, queued = L.rebvio_hip_kf_snapshot_point_cloud, L.rebvio_hip_kf_snapshot_point_cloud_async
    base = B.test_live_resources()
    nan = float("nan")
    for flt, text in (((2, 0.5, 0.0, 20.0), "rho_min must be > 0"), ((2, 0.5, 5.0, 4.0), "rho_min > rho_max"),
                      ((2, -0.1, 1e-3, 20.0), "max_rel_sigma must be >= 0"), ((2, nan, 1e-3, 20.0), "NaN"), ((2, 0.5, nan, 20.0), "NaN"),
                      ((2, 0.5, 1e-3, nan), "NaN")):
        f = B.CloudFilter(int(flt[0]), float(flt[1]), float(flt[2]), float(flt[3]))
        assert sync(snap.h, f, None, None, 0, C.byref(n)) == -3 and text in err(), flt
        assert queued(snap.h, f, None, C.byref(h)) == -3 and text in err() and not h.value, flt
    for k in (0, 4, 8, 9, 11, 12):
        v = np.concatenate([np.eye(3).reshape(9), np.zeros(3), [1.0]])
        v[k] = nan
        p = B.cloud_pose(v[:9], v[9:12], v[12])
        assert sync(snap.h, None, p, None, 0, C.byref(n)) == -3 and "NaN in the pose" in err(), k
        assert queued(snap.h, None, p, C.byref(h)) == -3 and "NaN in the pose" in err(), k
    assert sync(None, None, None, None, 0, C.byref(n)) == -3 and "null snapshot" in err()
    assert sync(snap.h, None, None, None, 0, None) == -3 and "null count" in err()
    assert sync(snap.h, None, None, None, -1, C.byref(n)) == -3 and "cap" in err()
    assert sync(snap.h, None, None, None, 5, C.byref(n)) == -3 and "points buffer" in err()
    assert queued(None, None, None, C.byref(h)) == -3 and "null" in err()
    assert queued(snap.h, None, None, None) == -3 and "null" in err()
    assert B.test_live_resources() == base            # no refused call touched the device
    q = snap.point_cloud_async()
    ctx.close()
    assert sync(snap.h, None, None, None, 0, C.byref(n)) == -10 and "destroyed" in err()
    assert queued(snap.h, None, None, C.byref(h)) == -10 and "destroyed" in err() and not h.value
    with pytest.raises(B.HipError) as e:
        q.wait()
    assert "error -10:" in str(e.value) and "destroyed" in str(e.value)
    q.release()
    snap.release()
    m.release()


def test_a_snapshot_released_right_after_the_queued_call(B):
    ctx, (m,) = sized_maps(B, 800)
    prs4, mt = random_snapshot(800, 23)
    pose = random_pose(5)
    want = np_kf_cloud(prs4, mt, ctx.p.fm, DEFAULT, pose)
    snap = planted(m, prs4, mt)
    q = snap.point_cloud_async(None, pose)
    snap.release()
    other = planted(m, *random_snapshot(800, 24))    # another snapshot may take the freed buffer's place at once
    assert_cloud_equal(q.wait(), want, "the snapshot was released behind the queued call")
    q.release()
    other.release()
    ctx.close()


# ---- the refusal table: every shared refusal with its code and whole text; which one wins when several apply ------

REFUSED = {
    "download": (lambda s: s.dsnap.download(), -10, DEAD_SNAPSHOT),
    "point_cloud": (lambda s: s.dsnap.point_cloud(cap=4), -10, DEAD_SNAPSHOT),
    "point_cloud_async": (lambda s: s.dsnap.point_cloud_async(), -10, DEAD_SNAPSHOT),
    "wins: the filter over a destroyed snapshot": (lambda s: s.dsnap.point_cloud(s.B.default_cloud_filter(rho_min=-1.0), cap=4), -3,
                                                   "kf_snapshot_point_cloud: filter rho_min must be > 0"),
    "wins: the filter over a destroyed snapshot, queued": (lambda s: s.dsnap.point_cloud_async(s.B.default_cloud_filter(rho_min=-1.0)), -3,
                                                           "kf_snapshot_point_cloud_async: filter rho_min must be > 0"),
}

@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusal_table(refusal_scene, case):
    """every refusal of the table with its return code and its whole rebvio_hip_last_error text; nothing is allocated"""
    assert_refused(refusal_scene, *REFUSED[case])


def test_releasing_a_snapshot_leaves_the_last_error_alone(B):
    """rebvio_hip_kf_snapshot_release, of a husk and of a live snapshot, writes no message"""
    assert_release_keeps_the_message(B, lambda ctx: ctx.detect_u8(np.full((120, 160), 128, np.uint8), 0).keyframe_snapshot())
