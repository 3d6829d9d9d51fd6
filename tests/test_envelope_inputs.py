"""CPU side of tests/test_envelope_gpu.py: its restatement of the distance-field rule per tile, and the preconditions its
crowded-tile cases assert, on the oracle alone."""
import numpy as np
import pytest

from support import DF_TILE_CAP, assert_crowded_and_sparse, df_tile_edge, noise_frames, tile_lower_bounds


def test_tile_edge_follows_the_tile_budget():
    assert df_tile_edge(480, 640) == 32 and df_tile_edge(2048, 2048) == 32   # 64 x 64 = 4096 tiles: still 32
    assert df_tile_edge(2112, 2048) == 64 and df_tile_edge(1900, 2304) == 64 and df_tile_edge(2548, 4096) == 64


def test_tile_counts_of_a_hand_made_map(orc_mod):
    """Three keylines on a 96 x 64 frame with 32-pixel tiles (3 x 2): a horizontal segment through all three tiles of the upper
    row, a vertical one down the middle column, and one under the map's threshold, which writes nothing."""
    kl = np.zeros(3, orc_mod.KEYLINE_DTYPE)
    kl["pos"] = [(48.0, 10.0), (40.0, 30.0), (80.0, 50.0)]
    kl["gradient"] = [(2.0, 0.0), (0.0, 3.0), (0.3, 0.4)]
    kl["gradient_norm"] = [2.0, 3.0, 0.5]
    lb = tile_lower_bounds(kl, 1.0, 64, 96, 40, 32)
    # keyline 0: columns 8..87 of row 10; keyline 1: rows -10..69 of column 40, clipped to 0..63; keyline 2: skipped
    assert lb.tolist() == [[1, 2, 1], [0, 1, 0]]
    # without a threshold the slanted one counts too: cells (80 + 0.6 r, 50 + 0.8 r), inside the frame for r = -40..16: columns
    # 56..90, rows 18..63; it leaves column 63 in row 28 and enters row 32 in column 66
    lb = tile_lower_bounds(kl, 0.0, 64, 96, 40, 32)
    assert lb.tolist() == [[1, 3, 2], [0, 1, 1]]
    # search_range 5: columns 43..52 / rows 25..34
    assert tile_lower_bounds(kl, 1.0, 64, 96, 5, 32).tolist() == [[0, 2, 0], [0, 1, 0]]


def test_tile_counts_bound_the_oracles_own_field(orc_mod, small_stream):
    """On a real map: a tile's cells are won by keylines that the helper counted for it, so the distinct winners of a tile
    never outnumber its count, and a tile has cells exactly where its count is not zero."""
    frames, cam = small_stream
    orc = orc_mod.Oracle(orc_mod.default_params(cam.height, cam.width, keylines_ref=1500, keylines_max=2000))
    for i in range(2):
        om = orc.detect_u8(frames[i], i * 50000)
    orc.build_distance_field(om)
    ids, _ = orc.distance_field()
    lb = tile_lower_bounds(om.keylines(), om.threshold, cam.height, cam.width, 40, 32)
    for ty in range(lb.shape[0]):
        for tx in range(lb.shape[1]):
            won = np.unique(ids[ty * 32:ty * 32 + 32, tx * 32:tx * 32 + 32])
            won = won[won >= 0]
            assert len(won) <= lb[ty, tx] and (len(won) > 0) == (lb[ty, tx] > 0), (ty, tx, len(won), lb[ty, tx])
    assert lb.max() > 100


@pytest.mark.parametrize("size", [(640, 480), (192, 144)])
def test_noise_frames_crowd_some_tiles_and_not_others(orc_mod, size):
    W, H = size
    orc = orc_mod.Oracle(orc_mod.default_params(H, W))
    for i, f in enumerate(noise_frames(W, H, 2, 5)):
        lb = assert_crowded_and_sparse(orc.detect_u8(f, i * 50000), H, W, what=f"{W}x{H} frame {i}")
        assert lb.max() > DF_TILE_CAP + 100   # not a marginal case
