"""EdgeMap::forwardMatch (edge_map.cpp:73-99) on crafted maps: the oracle against a closed-form statement (CPU only).

The GPU tests of tests/test_forward_match_gpu.py compare the library with the oracle's forward_match bit for bit, and the
library does not walk the old map in index order as the reference does: it lets the largest (rho, old index) key win per target
(track.hip: k_forward_keys / the last tryVel evaluation, xrv_apply). So the oracle's walk is pinned here first, against the rule
the walk amounts to, stated without a walk:

  * a target ends with the fields of its writer of largest rho, the largest index among equals,
  * if the target came in unmatched, or its own rho is not larger than that writer's; otherwise it stays bit for bit as it was;
  * the returned count is the number of writes of the sequential walk (a target written twice counts twice): a writer writes
    when its rho is at least the largest rho in front of it - the earlier writers' and, for a target that came in matched, the
    target's own; the first writer of an unmatched target always writes.

The crafted maps - many writers per target, laid out contiguously and with stride 6, four rho patterns, targets pre-set around
the winner's rho - are built by the helpers of tests/support.py, which the GPU file uses too. Each helper asserts on its own
result that the map holds what it claims.
"""
import numpy as np
import pytest

from conftest import params_for
from support import (DONOR, KW_TRACK, LAYOUTS, PATTERNS, RERUN_VELS, START_VELS, WG, assert_donor_pair, assert_keylines_equal,
                     behind_the_camera, craft_donor_copies, craft_writers, forward_match_closed_form, kept_and_overwritten,
                     preset_targets, targets_of, winner_of, writers_by_target)


# ---- the oracle against the closed form ----------------------------------------------------------------------------------
def oracle_stage(orc_mod, stream):
    """The oracle's side of support.warm(…, 3) and what the GPU file does next: three warm-up pairs, the keyline sums in
    the kernels' order from then on, the distance field of the fresh newest map. Returns (oracle, the three newest maps)."""
    frames, cam = stream
    orc = orc_mod.Oracle(params_for(orc_mod, cam, **KW_TRACK))
    maps = [orc.detect_u8(frames[0], 0)]
    for i in range(1, 5):
        maps.append(orc.detect_u8(frames[i], i * 50000))
        if i < 4:
            orc.track_pair(maps[-2], maps[-1])
    orc.set_sum_order("device")
    orc.build_distance_field(maps[-1])
    return orc, maps[-3:]


@pytest.fixture(scope="module")
def stage(orc_mod, small_stream):
    """The pair after three warm-up pairs on the oracle, after its minimizeVel: (oracle, old map, fresh new map)."""
    orc, (_, old, new) = oracle_stage(orc_mod, small_stream)
    orc.minimize_vel(old)
    return orc, old, new


def run_oracle(orc, old_map, new_map, old, new):
    """forward_match on clones of the stage's maps that hold the crafted arrays: (result, count)"""
    o, n = old_map.clone(), new_map.clone()
    o.set_keylines(old)
    n.set_keylines(new)
    count = orc.forward_match(o, n)
    assert_keylines_equal(o.keylines(), old, "the old map is read only")
    return n.keylines(), count


def test_natural_pair_has_few_writers_per_target(stage):
    """What the natural frames give this step (the reason for the crafted maps): on the pair of the stage at most 3 writers per
    target and no target whose best rho is tied; the closed form agrees with the oracle there too."""
    orc, old_map, new_map = stage
    old, new = old_map.keylines(), new_map.keylines()
    assert (new["match_id"] == -1).all()
    by_target = writers_by_target(old)
    most = max(len(m) for m in by_target.values())
    multi = sum(len(m) >= 2 for m in by_target.values())
    tied = sum((old["rho"][m] == old["rho"][m].max()).sum() >= 2 for m in by_target.values() if len(m) >= 2)
    print(f"natural pair: {len(by_target)} targets, {multi} with two or more writers, at most {most} per target, {tied} with a tied best rho")
    assert len(by_target) > 1000 and multi > 100 and most <= 3 and tied == 0
    got, count = run_oracle(orc, old_map, new_map, old, new)
    want, want_count = forward_match_closed_form(old, new)
    assert_keylines_equal(got, want, "natural pair")
    assert count == want_count


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_many_writers_into_unmatched_targets(stage, layout, pattern):
    """Section a's maps: groups of 1 .. 600 writers per target, every target unmatched. The winner's fields in every target,
    every other keyline of the new map and every other field of a target as it was, and the count of the sequential walk."""
    orc, old_map, new_map = stage
    new = new_map.keylines()
    assert (new["match_id"] == -1).all()
    old, groups = craft_writers(old_map.keylines(), len(new), layout, pattern)
    got, count = run_oracle(orc, old_map, new_map, old, new)
    want, want_count = forward_match_closed_form(old, new)
    assert_keylines_equal(got, want, f"{layout}, {pattern}")
    assert count == want_count, (count, want_count)
    assert len(groups) <= count <= sum(len(m) for _, m in groups)
    if pattern == "equal":    # every writer writes: the walk's count is the number of writers
        assert count == sum(len(m) for _, m in groups)
        assert all(got["match_id"][t] == m[-1] for t, m in groups)
    targets = np.array([t for t, _ in groups])
    assert (got["match_id"][targets] >= 0).all() and int((got["match_id"] >= 0).sum()) == len(groups)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_many_writers_into_matched_targets(stage, layout, pattern):
    """Section b's maps: the same groups into targets that are already matched, their rho above, equal to, one ulp above, one ulp
    below and well below the winning writer's. At least 20 targets keep every bit and at least 20 are overwritten."""
    orc, old_map, new_map = stage
    old, groups = craft_writers(old_map.keylines(), new_map.size(), layout, pattern)
    new, kinds = preset_targets(new_map.keylines(), old, groups)
    got, count = run_oracle(orc, old_map, new_map, old, new)
    want, want_count = forward_match_closed_form(old, new)
    assert_keylines_equal(got, want, f"{layout}, {pattern}")
    assert count == want_count, (count, want_count)
    kept, over = kept_and_overwritten(new, got, groups)
    print(f"{layout}, {pattern}: {kept} targets kept, {over} overwritten, count {count}")
    assert kept >= 20 and over >= 20, (kept, over)
    for (t, m), kind in zip(groups, kinds):
        w = winner_of(old, m)
        if kind in ("above", "ulp_above"):
            assert got["match_id"][t] == new["match_id"][t] != w and got["rho"][t] == new["rho"][t] > old["rho"][w], (t, kind)
        else:
            assert got["match_id"][t] == w and got["matches"][t] == old["matches"][w] + 1 and got["rho"][t] == old["rho"][w], (t, kind)


def test_second_forward_match_from_an_older_map(orc_mod, small_stream):
    """The reference's rule on natural maps: a second forwardMatch into the same new map, from the map one frame older, keeps
    the targets whose first match holds the larger rho. Closed form against the oracle; hundreds are kept and hundreds overwritten."""
    orc, (older, old, new) = oracle_stage(orc_mod, small_stream)
    orc.minimize_vel(old)
    orc.forward_match(old, new)
    first = new.keylines()
    orc.minimize_vel(older)
    ko = older.keylines()
    by_target = writers_by_target(ko)
    want, want_count = forward_match_closed_form(ko, first)
    count = orc.forward_match(older, new)
    got = new.keylines()
    assert_keylines_equal(got, want, "second forwardMatch")
    assert count == want_count
    kept, over = kept_and_overwritten(first, got, [(t, m) for t, m in by_target.items() if first["match_id"][t] >= 0])
    print(f"second forwardMatch from the older map: {len(by_target)} targeted, {kept} kept, {over} overwritten")
    assert kept >= 100 and over >= 100, (kept, over)


def test_a_second_minimize_vel_untargets_keylines_of_the_first(orc_mod, small_stream):
    """Section c's precondition: minimizeVel from 0, then from another start velocity, on the same old map. Targets of the first
    run that no keyline forwards to after the second (93 from (0, 0, -0.06), 1161 from (0.2, 0.1, 0) of 1430): a forwardMatch
    that still knew the first run would hand each of them a match."""
    orc, (_, old, new) = oracle_stage(orc_mod, small_stream)
    orc.minimize_vel(old)
    first = targets_of(old.keylines())
    for vel0 in RERUN_VELS:
        orc.minimize_vel(old, vel0)
        gone = len(first - targets_of(old.keylines()))
        print(f"second minimizeVel from {vel0}: {gone} of {len(first)} targets untargeted")
        assert gone >= 50, (vel0, gone)


def test_start_velocities_give_the_accept_masks(orc_mod, small_stream):
    """Section d's preconditions: the oracle's accept mask per start velocity, and that (0, 0, -0.9) sends evaluated keylines
    through z_p <= 0 in the first evaluation (733 of them; none at the other three)."""
    orc, (_, old, new) = oracle_stage(orc_mod, small_stream)
    for vel0, mask in START_VELS:
        ro = orc.minimize_vel(old, vel0)
        behind = behind_the_camera(old.keylines(), old.threshold, ro["sigma_rho_min"], vel0[2])
        print(f"minimizeVel from {vel0}: mask {ro['accept_mask']:05b}, {behind} keylines with z_p <= 0 at the start")
        assert f"{ro['accept_mask']:05b}" == mask, (vel0, ro["accept_mask"])
        assert behind >= 20 if vel0[2] == -0.9 else behind == 0, (vel0, behind)


@pytest.mark.parametrize("varied", [False, True], ids=["equal_rho", "varied_rho"])
def test_donor_copies_forward_to_one_target_through_a_pair(orc_mod, small_stream, varied):
    """Section e's precondition: with 300 old keylines made copies of keyline 936 the pair 3 -> 4 ends with status 0 and 1847
    matches, and all 301 forward to target 950, from 8 workgroups of 256."""
    frames, cam = small_stream
    orc = orc_mod.Oracle(params_for(orc_mod, cam, **KW_TRACK))
    orc.set_sum_order("device")
    maps = [orc.detect_u8(frames[0], 0)]
    for i in range(1, 5):
        maps.append(orc.detect_u8(frames[i], i * 50000))
        if i < 4:
            orc.track_pair(maps[-2], maps[-1])
    old, idx = craft_donor_copies(maps[-2].keylines(), DONOR, varied)
    maps[-2].set_keylines(old)
    po = orc.track_pair(maps[-2], maps[-1])
    t, m = assert_donor_pair(po, maps[-2].keylines(), idx, varied)
    print(f"donor {DONOR}: status {po.status}, {po.klm_num} matches, {len(m)} writers onto target {t} from {len(np.unique(m // WG))} workgroups")
    assert set(idx.tolist()) <= set(m.tolist()) and DONOR in m
