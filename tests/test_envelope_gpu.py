"""The accepted image-size envelope and crowded distance-field tiles, on the GPU against the oracle.

rebvio_hip_create accepts 32x32 .. 4096 columns x 2548 rows, keylines_max up to 65 536 and search_range up to 255; the
other GPU files stay inside 2048 columns, 960 rows and search_range 40. Here each code path that only the rest of the
envelope reaches is launched once and compared bit for bit (these stages are bit-exact by design):

  A  a size grid - the one-lane row walk of rowscan_body (more than 2048 columns), 64-pixel distance-field tiles (more than
     4096 tiles of 32 x 32), the column scan at the whole LDS of a CU (2548 rows), the smallest frames;
  B  distance-field tiles crossed by more than kDfTileCap = 512 keyline segments (rebuilt by df_rowrange_body), with the
     crowding asserted on the oracle's map alone before anything is compared, and search_range 1 / 10 / 100 / 255;
  C  whole pair steps at 2304x1900 and 4096x2548 with a full 65 536-keyline map;
  D  the colour / packed-YUV first pass and the lens-model front end at 2300 columns.

Large synthetic frames are a quarter-size synth stream enlarged 4x (np.kron): rendering 4096x2548 directly takes minutes.
"""
import numpy as np
import pytest

from conftest import params_for
from support import B  # noqa: F401
from support import (BGRA8, DF_TILE_CAP, EUROC_D, KW_C2, NAMES, RGB8, UYVY, assert_crowded_and_sparse, assert_keylines_equal,
                     assert_pipeline_bit_identical, bits_equal, colourise, df_tile_edge, enlarged_stream, noise_frames, pair_tuple,
                     record_words, run_stream, tile_lower_bounds)

pytestmark = pytest.mark.gpu

KW_FULL = dict(keylines_ref=60000, keylines_max=65536)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def mixed_frames(width, height, n=2, seed=0):
    """Frames with sparse and crowded regions: the enlarged synthetic stream, with squares of uniform noise (fresh in every
    frame) on a coarse grid and in the bottom right corner. Noise saturates the keyline budget within a few rows, so the squares
    stay a small share of the frame and the map still reaches the last rows."""
    frames, cam = enlarged_stream(width, height, n)
    rng = np.random.default_rng(seed + 7919 * width + height)
    side = 96
    for f in frames:
        for y in list(range(20, height - side, 700)) + [height - side]:
            for x in list(range(40, width - side, 900)) + [width - side]:
                y0, x0 = max(y, 0), max(x, 0)
                f[y0:y0 + side, x0:x0 + side] = rng.integers(0, 256, f[y0:y0 + side, x0:x0 + side].shape)
    return frames, cam


# ---- comparisons ------------------------------------------------------------------------------------------------------
def assert_field_equal(orc, ctx, om, gm, what):
    orc.build_distance_field(om)
    ctx.build_distance_field(gm)
    ido, dso = orc.distance_field()
    idg, dsg = ctx.distance_field()
    assert np.array_equal(ido, idg), f"{what}: field ids differ in {(ido != idg).sum()} cells, first {np.argwhere(ido != idg)[:3].tolist()}"
    sel = ido >= 0
    assert np.array_equal(dso[sel], dsg[sel]), f"{what}: field distances differ in {(dso[sel] != dsg[sel]).sum()} cells"
    return int(sel.sum())


def assert_detect_equal(om, gm, rows, cols, what):
    assert_keylines_equal(om.keylines(), gm.keylines(), what=what)
    assert np.array_equal(om.mask(rows, cols), gm.mask()), f"{what}: dense mask"
    assert bits_equal(np.float32(om.threshold), np.float32(gm.threshold)), (what, om.threshold, gm.threshold)


# ---- A: the size grid ---------------------------------------------------------------------------------------------------
SIZE_GRID = [(2052, 64), (2303, 40), (4096, 48), (4095, 33), (2048, 2112), (2300, 1900), (1700, 2548), (4096, 2548),
             (32, 32), (33, 35), (4096, 32), (35, 2548)]


def _grid_frames(W, H, n):
    if (W, H) == (4096, 48):
        # the first pass's integer row sums at their largest: near-white pixels, as test_first_row_pass_is_exact_on_wide_bright_frames
        rng = np.random.default_rng(W)
        frames = np.stack([rng.integers(200, 256, (H, W)).astype(np.uint8) for _ in range(n)])
        frames[1][:, ::3] = 255
        return frames
    return mixed_frames(W, H, n)[0]


@pytest.mark.parametrize("size", SIZE_GRID, ids=[f"{w}x{h}" for w, h in SIZE_GRID])
def test_size_grid_scale_space_detect_and_field(orc_mod, B, size):
    """One oracle and one context per size: (i) the scale space of an fp32 noise image (the fp32 row pass), (ii) detection of
    consecutive u8 frames (the u8 and box-average row passes; the later frames run the threshold servo and reuse a map) with
    every keyline field, the dense mask and the threshold, (iii) the distance field of every map. 2052 = first width past the
    wave form of the row pass, 2303 = lane walk with a padded pitch, 4096 / 4095 = widest, 2048x2112 = first 64-pixel tiles,
    2300x1900 = both, 2548 rows = column scan at 160 KiB of LDS, 32x32 = smallest.
    The frames of more than a megapixel would fill 65 536 keylines long before their last row at the default threshold, so
    they start the servo high (threshold 0.06, keylines_ref 40 000) and take three frames: a sparse map, a medium one - both
    down to the last rows - and, for all but the largest, one truncated at keylines_max with tiles over the list capacity
    (checked on the oracle with this recipe: 2 184..7 295, 14 113..45 644, 35 736..65 536 keylines)."""
    W, H = size
    big = W * H > 1 << 20
    kw = dict(KW_FULL, keylines_ref=40000, threshold=0.06) if big else dict(keylines_ref=12000, keylines_max=16000)
    orc = orc_mod.Oracle(orc_mod.default_params(H, W, **kw))
    ctx = B.Context(B.default_params(H, W, **kw))
    rng = np.random.default_rng(W * 4099 + H)
    img = rng.integers(0, 256, (H, W)).astype(np.float32) * np.float32(3.0)
    so, sg = orc.scale_space(img), ctx.scale_space(img)
    for k in ("scale0", "scale1", "dog", "mag"):
        assert bits_equal(so[k], sg[k]), f"{W}x{H} {k}: {(so[k].view(np.uint32) != sg[k].view(np.uint32)).sum()} pixels differ"
    del so, sg
    sizes, last_row = [], 0.0
    for i, f in enumerate(_grid_frames(W, H, 3 if big else 2)):
        om, gm = orc.detect_u8(f, i * 50000), ctx.detect_u8(f, i * 50000)
        assert_detect_equal(om, gm, H, W, f"{W}x{H} frame {i}")
        assert_field_equal(orc, ctx, om, gm, f"{W}x{H} frame {i}")
        sizes.append(om.size())
        last_row = max(last_row, float(om.keylines()["pos"][:, 1].max()))
        gm.release()
    # the inputs do what they are for (oracle side only): keylines down to the last rows, and not a handful of them
    assert last_row > H - 8 and min(sizes) > 100, (W, H, sizes, last_row)
    ctx.close()


# ---- B: crowded tiles and search ranges ---------------------------------------------------------------------------------


@pytest.mark.parametrize("case", ["noise-640x480", "noise-192x144", "enlarged-2304x1900"])
def test_crowded_tiles_fall_back_to_the_row_range(orc_mod, B, case):
    """A tile crossed by more than 512 keyline segments drops its list and is rebuilt from its candidate rows (df_lists_body ->
    df_rowrange_body). Uniform noise crosses the cap easily, and the map truncated at keylines_max leaves the lower tiles
    uncrowded, so both branches run in one launch; the enlarged synthetic stream does the same with 64-pixel tiles. Both are
    asserted on the oracle's map before the fields are compared."""
    if case == "enlarged-2304x1900":
        W, H, kw = 2304, 1900, dict(KW_FULL)
        frames = enlarged_stream(W, H, 2)[0]
    else:
        W, H = (640, 480) if case == "noise-640x480" else (192, 144)
        kw = {}  # the default budget: 12 000 / 16 000
        frames = noise_frames(W, H, 2, 5)
    orc = orc_mod.Oracle(orc_mod.default_params(H, W, **kw))
    ctx = B.Context(B.default_params(H, W, **kw))
    for i, f in enumerate(frames):
        om, gm = orc.detect_u8(f, i * 50000), ctx.detect_u8(f, i * 50000)
        lb = assert_crowded_and_sparse(om, H, W, what=f"{case} frame {i}")
        print(f"{case} frame {i}: {om.size()} keylines, T = {df_tile_edge(H, W)}, peak {lb.max()}, {(lb > DF_TILE_CAP).sum()} of {lb.size} tiles over {DF_TILE_CAP}")
        assert_detect_equal(om, gm, H, W, f"{case} frame {i}")
        assert_field_equal(orc, ctx, om, gm, f"{case} frame {i}")
    ctx.close()


def test_crowded_tiles_in_a_batch(orc_mod, B, c2_stream):
    """The batched kernels (k_join_edges_b, k_df_lists_b) share the body but not the argument plumbing: two lanes, one fed a
    noise stream (crowded tiles in every map, asserted on the oracle), one the synthetic stream, against stand-alone contexts and
    against the oracle with its sums in the kernels' order. A batch hands out pair records, not maps: the field is compared
    through everything the tracker reads from it (matches, sums, counters - every word of every record)."""
    frames, cam = c2_stream
    n = 6
    noise = noise_frames(cam.width, cam.height, 1, 11)[0]
    # a noise image that moves one pixel per frame, so that the tracker has something to follow
    streams = [np.stack([np.roll(noise, k, axis=1) for k in range(n)]), np.ascontiguousarray(frames[:n])]
    order = np.arange(n)
    npx = cam.width * cam.height
    want = []
    for s in range(2):
        orc = orc_mod.Oracle(params_for(orc_mod, cam, **KW_C2))
        orc.set_sum_order("device")
        prev, recs, sparse = None, [], False
        for k in order:
            m = orc.detect_u8(streams[s][k], int(k) * 50000)
            lb = tile_lower_bounds(m.keylines(), m.threshold, cam.height, cam.width, 40, df_tile_edge(cam.height, cam.width))
            if s == 0:
                assert lb.max() > DF_TILE_CAP, (k, lb.max())
            sparse = sparse or bool(((lb > 0) & (lb <= DF_TILE_CAP // 2)).any())
            if prev is not None:
                recs.append(orc.track_pair(prev, m))
            prev = m
        assert sparse, s
        want.append(recs)
    bat = B.Batch(params_for(B, cam, **KW_C2), 2)
    devs = [bat.lanes[s].upload_frames(streams[s]) for s in range(2)]
    got = [[], []]
    for k in order:
        outs, nks = bat.push_u8_device([d + int(k) * npx for d in devs], int(k) * 50000)
        for s in range(2):
            if outs[s].status >= 0:
                got[s].append((record_words(outs[s]), pair_tuple(outs[s], nks[s])))
    for outs, nks in bat.flush():
        for s in range(2):
            got[s].append((record_words(outs[s]), pair_tuple(outs[s], nks[s])))
    bat.close()
    for s in range(2):
        ctx = B.Context(params_for(B, cam, **KW_C2))
        dev = ctx.upload_frames(streams[s])
        alone = [pair_tuple(o, nk) for o, nk in run_stream(ctx, dev, order, npx)]
        ctx.close()
        assert len(got[s]) == len(alone) == len(want[s]) == n - 1
        for k in range(n - 1):
            assert got[s][k][1] == alone[k], (s, k)
            wo = record_words(want[s][k])
            assert np.array_equal(wo, got[s][k][0]), (s, k, np.flatnonzero(wo != got[s][k][0])[:8])


@pytest.mark.parametrize("search_range", [1, 10, 100, 255])
def test_distance_field_with_other_search_ranges(orc_mod, B, small_stream, search_range):
    """search_range sets df_nr, the (r_lo + 256) << 16 packing of the tile entries and the sequence bits of the field key
    (keylines_max * 2 * search_range < 2^23: 2000 keylines leave room up to the accepted maximum of 255; create also wants
    search_range + 2 * pixel_uncertainty_match + 2 <= 260, so the match uncertainty goes down to 1 there)."""
    frames, cam = small_stream
    kw = dict(keylines_ref=1500, keylines_max=2000, search_range=float(search_range), pixel_uncertainty_match=1.0)
    assert kw["keylines_max"] * 2 * search_range < 1 << 23
    orc = orc_mod.Oracle(params_for(orc_mod, cam, **kw))
    ctx = B.Context(params_for(B, cam, **kw))
    for i in range(3):
        om, gm = orc.detect_u8(frames[i], i * 50000), ctx.detect_u8(frames[i], i * 50000)
        assert_detect_equal(om, gm, cam.height, cam.width, f"search_range {search_range} frame {i}")
        cells = assert_field_equal(orc, ctx, om, gm, f"search_range {search_range} frame {i}")
        assert cells >= om.size() > 1000
    ctx.close()


# ---- C: a pair step outside the tested box ---------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(2304, 1900), (4096, 2548)], ids=["2304x1900", "4096x2548"])
def test_pair_steps_at_the_large_sizes(orc_mod, B, size):
    """Three pairs with a 65 536-keyline budget where the dense mask and the field have up to 10.4 M cells: four frames of a
    quarter-size synth stream enlarged 4x (camera fm * 4, c * 4 + 1.5), keylines_ref 60 000. Precondition on the oracle alone:
    every pair ends with status 0 and at least global_min_matches_threshold LM matches. Then the comparison of
    test_whole_pipeline_is_bit_identical_with_the_sums_in_one_order."""
    W, H = size
    frames, cam = enlarged_stream(W, H, 4)
    assert_pipeline_bit_identical(orc_mod, B, frames, cam, np.arange(4), KW_FULL, 5000, what=f"{W}x{H}", every_pair_tracks=True)


# ---- D: the other frame entry points past 2048 columns ---------------------------------------------------------------------
def test_colour_and_lens_entry_points_on_a_wide_frame(orc_mod, B):
    """k_rowscan_px (one 3-byte, one 4-byte and one packed-YUV format) and the lens-model front end followed by the fp32 first
    pass, at 2300 x 64: the row pass walks each row with one lane there."""
    W, H = 2300, 64
    frames, cam = mixed_frames(W, H, 2, seed=3)
    kw = dict(fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=6000, keylines_max=8000)
    px = colourise(frames, 13)
    for fmt in (RGB8, BGRA8, UYVY):
        col, grey = px[fmt]
        orc = orc_mod.Oracle(orc_mod.default_params(H, W, **kw))
        ctx = B.Context(B.default_params(H, W, **kw))
        for i in range(2):
            om, gm = orc.detect_u8(grey[i], i * 50000), ctx.detect_px(col[i], fmt, i * 50000)
            assert_detect_equal(om, gm, H, W, f"{NAMES[fmt]} frame {i}")
        assert om.size() > 1000
        ctx.close()
    orc = orc_mod.Oracle(orc_mod.default_params(H, W, **kw))
    ctx = B.Context(B.default_params(H, W, **kw))
    K = (cam.fm, cam.fm, cam.cx, cam.cy)
    ctx.set_undistort(*K, EUROC_D)
    for i in range(2):
        und = orc.front_end_u8(frames[i], *K, EUROC_D)
        assert bits_equal(und, ctx.front_end_u8(frames[i])), f"front end, frame {i}"
        om, gm = orc.detect(und, i * 50000), ctx.detect_u8_host(frames[i], i * 50000)
        assert_detect_equal(om, gm, H, W, f"lens model frame {i}")
    assert om.size() > 1000
    ctx.close()
