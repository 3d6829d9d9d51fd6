"""Large and wrong rotation priors, on the CPU oracle alone: what tests/test_large_rotations_gpu.py takes for granted when it
holds the library to the oracle there. A gyro hands over 0.1 - 0.3 rad per frame on a fast turn and anything on a glitch; the
rest of the suite rotates by milliradians. Here: the oracle survives a wrong prior in mid-stream and tracks again behind it
(WRONG_PRIORS, CONSECUTIVE), tracks a true turn of 6 degrees per frame with its prior and not without (FAST_TURNS), and the
crafted maps put rotateKeylines (edge_map.cpp:58-71) on every edge it has: a rotated z of +0, -0, a denormal, a negative one, and
depths of 0, -1, inf, NaN and the two clamps going in. Everything at 192x144 with KW_TRACK, eight frames, sums in device order;
the tables in tests/support.py carry what was measured."""
import numpy as np
import pytest

from conftest import params_for
from support import (BAD_PAIR, CONSECUTIVE, CONSECUTIVE_PAIRS, CRAFT_ROTATIONS, CRAFT_SIZES, FAST_TURNS, KW_TRACK, N_TURN, TURN_MIN_KLM,
                     WRONG_PRIORS, craft_rotation_map, oracle_pairs, record_words, rotated_z, rotation_classes, turn_stream, w_id, words,
                     wrong_prior_rotations)


def pairs(orc_mod, frames, cam, R):
    return [po for po, _ in oracle_pairs(orc_mod, cam, frames, R, **KW_TRACK)]


@pytest.mark.parametrize("elsewhere", [None, "gyro"], ids=["no-other-prior", "small-priors-elsewhere"])
@pytest.mark.parametrize("w", list(WRONG_PRIORS), ids=w_id)
def test_oracle_survives_a_wrong_prior_in_mid_stream(orc_mod, w, elsewhere):
    """One wrong prior rodrigues(w) on pair 3 -> 4: that pair ends with the status and klm_num of the table, each of the three
    pairs behind it with status 0 and at least 1500 matches, and all four records differ from the run without the bad prior."""
    frames, cam, _ = turn_stream()
    status, klm_none, klm_gyro = WRONG_PRIORS[w]
    got = pairs(orc_mod, frames, cam, wrong_prior_rotations({BAD_PAIR: w}, elsewhere=elsewhere))
    base = pairs(orc_mod, frames, cam, wrong_prior_rotations({}, elsewhere=elsewhere))
    assert len(got) == N_TURN - 1
    assert (got[BAD_PAIR].status, got[BAD_PAIR].klm_num) == (status, klm_gyro if elsewhere else klm_none)
    for k in range(N_TURN - 1):
        same = np.array_equal(record_words(got[k]), record_words(base[k]))
        assert same == (k < BAD_PAIR), (k, same)
        if k != BAD_PAIR:
            assert got[k].status == 0 and got[k].klm_num >= 1500, (k, got[k].status, got[k].klm_num)
    assert all(po.status == 0 for po in base)


def test_oracle_survives_wrong_priors_on_consecutive_pairs(orc_mod):
    frames, cam, _ = turn_stream()
    got = pairs(orc_mod, frames, cam, wrong_prior_rotations(CONSECUTIVE))
    assert [(po.status, po.klm_num) for po in got] == CONSECUTIVE_PAIRS


@pytest.mark.parametrize("yaw", list(FAST_TURNS))
def test_oracle_on_the_fast_turn_streams(orc_mod, yaw):
    """The scene of stream 0 turning by `yaw` degrees per frame (0.105 rad at 6), the true relative rotation as prior: every
    pair's klm_num is the table's, with and without the prior. At +6 the prior is what makes the stream trackable: 700 matches or
    more on every pair with it, fewer on at least five of seven without."""
    frames, cam, R = turn_stream(yaw)
    with_prior, without = pairs(orc_mod, frames, cam, R), pairs(orc_mod, frames, cam, None)
    assert all(po.status == 0 for po in with_prior + without)
    assert ([po.klm_num for po in with_prior], [po.klm_num for po in without]) == FAST_TURNS[yaw]
    if yaw == 6.0:
        assert min(FAST_TURNS[yaw][0]) >= TURN_MIN_KLM
        assert sum(k < TURN_MIN_KLM for k in FAST_TURNS[yaw][1]) >= 5
    for a, b in zip(with_prior, without):
        assert not np.array_equal(record_words(a), record_words(b))


@pytest.mark.parametrize("n", CRAFT_SIZES)
@pytest.mark.parametrize("name", list(CRAFT_ROTATIONS))
def test_crafted_maps_reach_every_edge_of_rotate_keylines(orc_mod, name, n):
    """craft_rotation_map under the exact matrices of 90 degrees about y and x and under UNDERFLOW_Z: the classes are there by
    count (from rotated_z, the statement of the product in numpy), and the oracle treats them as edge_map.cpp:62-69 says - a
    keyline whose rotated z is +-0 keeps pos_img, rho and sigma_rho bit for bit and still gets the rotated gradient; every other
    keyline is divided by its z, whatever that gives."""
    frames, cam, _ = turn_stream()
    R = CRAFT_ROTATIONS[name]
    orc = orc_mod.Oracle(params_for(orc_mod, cam, **KW_TRACK))
    m = orc.detect_u8(frames[0], 0)
    kl = craft_rotation_map(m.keylines(), n)
    c = rotation_classes(kl, R, cam.fm)
    if n >= 63:
        if name == "underflow":
            assert c["minus_zero"] >= 4 and c["plus_zero"] >= 4, c
        else:
            assert c["plus_zero"] >= 16 and c["denormal"] >= 8 and c["negative"] >= 16 and c["minus_zero"] == 0, c
        for f in ("rho", "sigma_rho"):
            assert all(c[f"{f}={v}"] >= 7 for v in (0.0, -1.0, np.inf, np.nan)), c
    else:
        assert c["plus_zero"] + c["negative"] == 1, c
    m.set_keylines(kl)
    orc.rotate(m, R)
    out = m.keylines()
    z = rotated_z(kl, R, cam.fm)
    kept = ((words(out["pos_img"]).reshape(-1, 2) == words(kl["pos_img"]).reshape(-1, 2)).all(1) & (words(out["rho"]) == words(kl["rho"])) &
            (words(out["sigma_rho"]) == words(kl["sigma_rho"])))
    assert kept[z == 0].all()
    with np.errstate(all="ignore"):
        want = (kl["rho"] / z).astype(np.float32)
    assert np.array_equal(words(out["rho"][z != 0]), words(want[z != 0]))
    g = kl["gradient"].astype(np.float64) @ np.asarray(R, np.float64)[:2, :2].T
    assert np.array_equal(out["gradient"], g.astype(np.float32))
    if n >= 63 and name != "underflow":   # what the division leaves behind: the inputs of every later float-to-int conversion
        assert np.isinf(out["pos_img"]).any() and (out["rho"] < 0).any() and np.isinf(out["sigma_rho"]).any() and np.isnan(out["sigma_rho"]).any()
