"""Everything a context, an edge map, a point cloud or a batch takes from the HIP runtime goes back when it is destroyed.

rebvio_hip_test_live_resources counts the device buffers, pinned buffers, events and streams the library holds in this process
(owned.hpp: one atomic, +1 per resource handed out, -1 per one given back). Every case reads it first and requires exactly that
value again at the end: the count is exact, so there is no tolerance. Frames staged with upload_frames are the caller's memory
(rebvio_hip_device_alloc) and are not counted."""
import time

import numpy as np
import pytest

from conftest import params_for
from support import B  # noqa: F401
from support import EUROC_D, vision_only_fusion

pytestmark = pytest.mark.gpu

KW = dict(keylines_ref=2500, keylines_max=3500, global_min_matches_threshold=50)  # as tests/cpp/test_map_lifetime.cpp


def _plain_round(B, frames, cam):
    """create, 8 device frames through the streaming driver, flush, destroy; returns (seconds create took, records delivered)"""
    npx = cam.width * cam.height
    t0 = time.perf_counter()
    ctx = B.Context(params_for(B, cam, **KW))
    t_create = time.perf_counter() - t0
    dev = ctx.upload_frames(frames)
    got = 0
    for k in range(8):
        out, _ = ctx.push_frame_u8_device(dev + k * npx, k * 50000)
        got += out.status >= 0
    got += len(ctx.flush())
    ctx.close()
    return t_create, got


def test_plain_context(B, small_stream):
    frames, cam = small_stream
    live = B.test_live_resources()
    ctx = B.Context(params_for(B, cam, **KW))
    assert B.test_live_resources() > live + 100     # the counter sees the context: streams, scan buffers, the pooled maps' arrays
    ctx.close()
    assert B.test_live_resources() == live
    _, got = _plain_round(B, frames, cam)
    assert got == 7
    assert B.test_live_resources() == live


def test_every_lazy_allocation_in_one_context(B, small_stream):
    frames, cam = small_stream
    npx = cam.width * cam.height
    lens = (cam.fm, cam.fm, cam.cx, cam.cy)
    live = B.test_live_resources()
    ctx = B.Context(params_for(B, cam, **KW))
    created = B.test_live_resources()
    dev = ctx.upload_frames(frames)
    host_map = ctx.detect_u8_host(frames[0], 0)                 # a host frame: the pinned ring and its events
    ring = B.test_live_resources()
    assert ring == created + 2 * 16                             # kPin slots, one event each; the pooled maps sufficed
    ctx.set_undistort(*lens, EUROC_D)
    first = B.test_live_resources()
    assert first == ring + 3                                    # the map and one undistorted frame per detect parity
    ctx.set_undistort(*lens, [0, 0, 0, 0, 0])                   # identity: the map is given back at once
    assert B.test_live_resources() == first - 1
    ctx.set_undistort(*lens, EUROC_D)
    assert B.test_live_resources() == first                     # re-setting allocates the map again and nothing else
    ctx.set_undistort(*lens, EUROC_D)
    assert B.test_live_resources() == first
    ctx.set_detection_mask(np.ones((cam.height, cam.width), np.uint8))
    ctx.set_detection_mask(np.ones((cam.height, cam.width), np.uint8))
    assert B.test_live_resources() == first + 1
    ctx.scale_space(frames[0].astype(np.float32))               # diag0 / diag1
    ctx.scale_space(frames[0].astype(np.float32))
    assert B.test_live_resources() == first + 3
    host_map.release()
    maps = [ctx.detect_u8_device(dev + k * npx, k * 50000) for k in range(3)]
    assert ctx.track_pair(maps[0], maps[1]).status == 0
    before_clouds = B.test_live_resources()
    assert before_clouds == first + 3                           # (three maps out of a pool of six: none was added)
    maps[1].point_cloud()                                       # cloud scratch, cloud stream, one pooled cloud
    q = ctx.point_cloud_async(maps[1])
    q.wait()
    q.release()
    assert B.test_live_resources() > before_clouds
    mid = ctx.track_pair_begin(maps[1], maps[2])                # bf_done / h_bf
    ctx.track_pair_finish_async(maps[1], maps[2], *vision_only_fusion(mid))
    assert ctx.track_pair_result()[3] == 0
    rgb = np.ascontiguousarray(np.repeat(frames[3][..., None], 3, -1))
    m = ctx.detect_px(rgb, B.PX_RGB8, 3 * 50000)               # a colour format
    assert m.size() > 100
    for k in range(4, 8):                                       # host-frame pushes, grey and colour; the streaming driver grows the pool
        out, _ = ctx.push_frame_u8(frames[k], k * 50000)
    rgb = np.ascontiguousarray(np.repeat(frames[8][..., None], 3, -1))
    ctx.push_frame_px(rgb, B.PX_RGB8, 8 * 50000)
    assert len(ctx.flush()) + (out.status >= 0) >= 1
    assert B.test_live_resources() > first + 3
    ctx.close()
    assert B.test_live_resources() == live
    for x in maps + [m]:                                        # (husks by now)
        x.release()
    assert B.test_live_resources() == live


def test_pool_growth(B, small_stream):
    frames, cam = small_stream
    npx = cam.width * cam.height
    live = B.test_live_resources()
    ctx = B.Context(params_for(B, cam, map_pool=4, **KW))
    dev = ctx.upload_frames(frames)
    base = B.test_live_resources()
    maps = []
    for k in range(7):
        maps.append(ctx.detect_u8_device(dev + k * npx, k * 50000))
        if k == 3:
            assert B.test_live_resources() == base              # the four pooled maps
    grown = B.test_live_resources()
    assert grown > base and (grown - base) % 3 == 0             # three fresh maps, the same number of resources each
    assert all(m.size() > 100 for m in maps)
    for m in maps:
        m.release()
    assert B.test_live_resources() == grown                     # released maps stay pooled
    ctx.close()
    assert B.test_live_resources() == live


def test_husks_hold_no_device_resources(B, small_stream):
    frames, cam = small_stream
    live = B.test_live_resources()
    ctx = B.Context(params_for(B, cam, **KW))
    m = ctx.detect_u8(frames[0], 0)
    assert m.size() > 100
    q = ctx.point_cloud_async(m)
    ctx.close()
    assert B.test_live_resources() == live                      # device resources go with the context, handles out or not
    L = B.lib()
    assert L.rebvio_hip_map_size(m.h) == -10
    assert "destroyed" in L.rebvio_hip_last_error().decode()
    with pytest.raises(B.HipError) as e:
        q.wait()
    assert "error -10:" in str(e.value)
    q.release()
    m.release()
    assert B.test_live_resources() == live


# "Two lanes, 6 steps, flush, batch_destroy; then the same with a lens model set on one lane": a batch refuses to step while
# only some of its lanes have a lens model, so the second half cannot run its 6 steps in that state. It is checked in two
# parts instead. test_batch[True] sets the model on lane 0, sees the step refused, sets it on lane 1 as well and runs the 6
# steps; test_batch_with_a_lens_model_on_one_lane_only destroys a batch in the one-lane state, without a step.
@pytest.mark.parametrize("lens", [False, True])
def test_batch(B, small_stream, lens):
    frames, cam = small_stream
    npx = cam.width * cam.height
    live = B.test_live_resources()
    bat = B.Batch(params_for(B, cam, **KW), 2)
    devs = [lane.upload_frames(frames) for lane in bat.lanes]
    if lens:                                                    # a model on one lane: its buffers exist, the step is refused
        bat.lanes[0].set_undistort(cam.fm, cam.fm, cam.cx, cam.cy, EUROC_D)
        with pytest.raises(B.HipError, match="every lane or on none"):
            bat.push_u8_device(devs, 0)
        bat.lanes[1].set_undistort(cam.fm, cam.fm, cam.cx, cam.cy, EUROC_D)
    got = 0
    for k in range(6):
        outs, _ = bat.push_u8_device([d + k * npx for d in devs], k * 50000)
        got += outs[0].status >= 0
    got += len(bat.flush())
    assert got == 5
    bat.close()
    assert B.test_live_resources() == live


def test_batch_with_a_lens_model_on_one_lane_only(B, small_stream):
    frames, cam = small_stream
    live = B.test_live_resources()
    bat = B.Batch(params_for(B, cam, **KW), 2)
    bat.lanes[1].set_undistort(cam.fm, cam.fm, cam.cx, cam.cy, EUROC_D)
    bat.close()
    assert B.test_live_resources() == live


def test_rejected_create_takes_nothing(B):
    live = B.test_live_resources()
    with pytest.raises(B.HipError) as e:
        B.Context(B.default_params(16, 640))
    assert "error -3:" in str(e.value)
    assert B.test_live_resources() == live


def test_ten_rounds_in_one_process(B, small_stream):
    frames, cam = small_stream
    live = B.test_live_resources()
    t = []
    for r in range(10):
        t_create, got = _plain_round(B, frames, cam)
        t.append(t_create)
        assert got == 7
        assert B.test_live_resources() == live, r
    print(f"rebvio_hip_create, mean of {len(t)} rounds: {1e3 * sum(t) / len(t):.2f} ms (min {1e3 * min(t):.2f}, max {1e3 * max(t):.2f})")
