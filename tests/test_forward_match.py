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
the winner's rho - are built by the helpers below, which the GPU file imports. Each helper asserts on its own result that the
map holds what it claims.
"""
import numpy as np
import pytest

from conftest import params_for

KW = dict(keylines_ref=1500, keylines_max=2500, global_min_matches_threshold=1)   # as tests/test_track_params_gpu.py
RHO_MIN, RHO_MAX = np.float32(1e-3), np.float32(20.0)  # types/keyline.hpp:13-14
GROUP_SIZES = (1, 2, 3, 63, 64, 65, 256, 257, 600)
N_FILL = 120           # further groups of 1, 2 and 3 writers: enough targets for every pre-set kind of section b
LAYOUTS = ("contiguous", "stride6")
PATTERNS = ("distinct", "equal", "shared_max", "clamps")
PRESETS = ("above", "equal", "ulp_above", "ulp_below", "well_below")   # the target's own rho against the winning writer's
WG = 256               # threads per workgroup of k_forward_keys; the LM kernels publish from 256, 512 or 1024
HANDED = ("rho", "sigma_rho", "matches", "match_id", "match_pos_img", "match_gradient", "match_gradient_norm", "match_id_keyframe")


def f32(x):
    return np.float32(x)


def ulp_up(x):
    return np.nextafter(f32(x), f32(np.inf), dtype=np.float32)


def ulp_down(x):
    return np.nextafter(f32(x), f32(-np.inf), dtype=np.float32)


# ---- the closed form ---------------------------------------------------------------------------------------------------
def writers_by_target(old):
    """dict target -> ascending old indices whose match_id_forward names it"""
    fwd = old["match_id_forward"]
    w = np.flatnonzero(fwd >= 0)
    order = np.argsort(fwd[w], kind="stable")
    w = w[order]
    cuts = np.flatnonzero(np.diff(fwd[w])) + 1
    return {int(fwd[g[0]]): g for g in np.split(w, cuts)} if len(w) else {}


def winner_of(old, members):
    """the writer of largest rho, the largest index among equals"""
    rho = old["rho"][members]
    return int(members[np.flatnonzero(rho == rho.max())[-1]])


def forward_match_closed_form(old, new):
    """(the new map after old->forwardMatch(new), the returned count), from the rule in this file's docstring"""
    out = new.copy()
    count = 0
    for t, members in writers_by_target(old).items():
        rho = old["rho"][members]
        matched = new["match_id"][t] >= 0
        front = np.maximum.accumulate(np.concatenate([[new["rho"][t] if matched else f32(-np.inf)], rho]))[:-1]
        count += int((rho >= front).sum())
        w = winner_of(old, members)
        if matched and new["rho"][t] > old["rho"][w]:
            continue
        out["rho"][t] = old["rho"][w]
        out["sigma_rho"][t] = old["sigma_rho"][w]
        out["matches"][t] = old["matches"][w] + np.uint32(1)
        out["match_id"][t] = w
        out["match_pos_img"][t] = old["pos_img"][w]
        out["match_gradient"][t] = old["gradient"][w]
        out["match_gradient_norm"][t] = old["gradient_norm"][w]
        out["match_id_keyframe"][t] = old["match_id_keyframe"][w]
    return out, count


def assert_bits_equal(a, b, what=""):
    assert len(a) == len(b)
    for f in a.dtype.names:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        if x.dtype.kind == "f":
            x, y = x.view(np.uint32), y.view(np.uint32)
        if not np.array_equal(x, y):
            bad = np.flatnonzero((x != y).reshape(len(a), -1).any(1))
            raise AssertionError(f"{what}: field {f} differs at {len(bad)} keylines, first {bad[:5]}: {a[f][bad[:3]]} vs {b[f][bad[:3]]}")


# ---- crafted maps ------------------------------------------------------------------------------------------------------
def group_slots(n_old, layout):
    """Old indices in the order the groups take them, index 0 and n_old - 1 kept back for the two sole writers. stride6: the
    indices of one residue class mod 6 after the other, so that consecutive members of a group lie six apart. A class of this
    map holds n_old / 6 indices, fewer than the 600 (and, behind it, the 257 and 256) writers ask for: such a group goes on in
    the next class, still six apart, and reaches over every workgroup of the map."""
    idx = np.arange(1, n_old - 1)
    if layout == "stride6":
        idx = np.concatenate([idx[idx % 6 == r] for r in range(6)])
    return idx


def group_rhos(pattern, g, size, rng):
    """rho of the `size` writers of group number g, in member order"""
    k = np.arange(size)
    base = f32(0.5) + f32(0.125) * f32(g % 5)
    if pattern == "equal":
        return np.full(size, base, np.float32)
    distinct = (base + f32(2.0 ** -10) * rng.permutation(size).astype(np.float32)).astype(np.float32)
    if pattern == "distinct":
        return distinct
    if pattern == "shared_max":   # the maximum twice, in the first and in the last quarter of the group (once in a group of one)
        top = f32(distinct.max() + f32(0.25))
        distinct[size // 8] = top
        distinct[size - 1 - size // 8] = top
        return distinct
    assert pattern == "clamps"
    if g % 4 == 0:      # every writer at kRhoMin: the smallest key of the claimed range wins
        return np.full(size, RHO_MIN, np.float32)
    if g % 4 == 1:      # every writer at kRhoMax
        return np.full(size, RHO_MAX, np.float32)
    if g % 4 == 2:      # both clamps among natural values: the last writer at kRhoMax wins
        return np.where(k % 3 == 0, RHO_MAX, np.where(k % 3 == 1, RHO_MIN, distinct)).astype(np.float32)
    distinct[k % 2 == 1] = RHO_MIN   # every second writer at kRhoMin under a natural winner
    return distinct


def craft_writers(old, n_new, layout, pattern):
    """The old map with match_id_forward = -1 everywhere but for crafted groups of writers, one target each: GROUP_SIZES, N_FILL
    small groups, and old index 0 and n_old - 1 as sole writers (the low word of index 0's key is 0). Targets 0 and n_new - 1 are
    among the targets. Returns (old map, list of (target, member indices)); asserts what the layout claims."""
    old = old.copy()
    n_old = len(old)
    rng = np.random.default_rng(len(layout) * 100 + len(pattern))
    sizes = sorted(GROUP_SIZES, reverse=True) + [1 + (j // 4) % 3 for j in range(N_FILL)]
    slots = group_slots(n_old, layout)
    assert sum(sizes) <= len(slots), (sum(sizes), n_old)
    n_groups = len(sizes) + 2
    targets = np.unique(np.linspace(0, n_new - 1, n_groups).astype(int))
    assert len(targets) == n_groups and targets[0] == 0 and targets[-1] == n_new - 1
    targets = targets[rng.permutation(n_groups)]    # (no relation between a group's place in the old map and its target's)
    old["match_id_forward"] = -1
    old["matches"] = (np.arange(n_old) % 7).astype(np.uint32)   # (what a wrong winner hands over differs in every field)
    old["match_id_keyframe"] = np.arange(n_old) % 11 - 1
    groups, at = [], 0
    for g, size in enumerate(sizes + [1, 1]):
        if g < len(sizes):
            members = np.sort(slots[at:at + size])
            at += size
        else:
            members = np.array([0 if g == len(sizes) else n_old - 1])
        old["match_id_forward"][members] = targets[g]
        old["rho"][members] = group_rhos(pattern, g, size, rng)
        groups.append((int(targets[g]), members))
    # what the layout claims, on the crafted array
    by_target = writers_by_target(old)
    assert len(by_target) == n_groups and all(np.array_equal(by_target[t], m) for t, m in groups)
    assert (old["rho"] >= RHO_MIN).all() and (old["rho"] <= RHO_MAX).all()
    assert int(old["match_id_forward"][0]) >= 0 and int(old["match_id_forward"][n_old - 1]) >= 0
    for t, m in groups:
        if len(m) >= 256:
            assert len(np.unique(m // WG)) >= 2, (len(m), m[0], m[-1])
        if layout == "stride6" and len(m) > 1:
            classes = [m[m % 6 == r] for r in np.unique(m % 6)]   # six apart within a class, at most two classes (one wrap)
            assert len(classes) <= 2 and all((np.diff(c) == 6).all() for c in classes), m[:8]
        if pattern == "distinct":
            assert len(np.unique(old["rho"][m])) == len(m)
        if pattern == "shared_max" and len(m) >= 2:
            top = np.flatnonzero(old["rho"][m] == old["rho"][m].max())
            assert len(top) == 2
            if len(m) >= 256:
                assert m[top[0]] // WG != m[top[1]] // WG
    if pattern == "clamps":
        wins = np.array([old["rho"][winner_of(old, m)] for _, m in groups])
        assert (wins == RHO_MIN).sum() >= 10 and (wins == RHO_MAX).sum() >= 10
    return old, groups


def preset_targets(new, old, groups):
    """The new map with every target of `groups` already matched (match_id >= 0) and its rho set against the winning writer's:
    above, equal, one ulp above, one ulp below, well below (PRESETS in turn). edge_map.cpp:83 keeps the first and the third.
    Returns (new map, kind per group)."""
    new = new.copy()
    kinds = []
    n_old = len(old)
    for j, (t, m) in enumerate(groups):
        wr = old["rho"][winner_of(old, m)]
        kind = PRESETS[j % len(PRESETS)]
        if kind == "above" and wr == RHO_MAX:   # (nothing in the claimed range lies above kRhoMax)
            kind = "equal"
        if kind == "well_below" and wr == RHO_MIN:
            kind = "equal"
        if kind == "ulp_above" and wr == RHO_MAX:
            kind = "ulp_below"
        if kind == "ulp_below" and wr == RHO_MIN:
            kind = "ulp_above"
        new["rho"][t] = {"above": f32(min(wr * f32(1.5), RHO_MAX)), "equal": wr, "ulp_above": ulp_up(wr), "ulp_below": ulp_down(wr),
                         "well_below": f32(max(wr * f32(0.5), RHO_MIN))}[kind]
        new["match_id"][t] = (7 * j + 3) % n_old
        new["sigma_rho"][t] = f32(0.0625) * f32(1 + j % 9)
        new["matches"][t] = 100 + j
        new["match_pos_img"][t] = (f32(j) - f32(40.5), f32(30.25) - f32(j))
        new["match_gradient"][t] = (f32(1.5), f32(-2.0))
        new["match_gradient_norm"][t] = f32(2.5)
        new["match_id_keyframe"][t] = j % 3 - 1
        kinds.append(kind)
    assert (new["rho"] >= RHO_MIN).all() and (new["rho"] <= RHO_MAX).all()
    return new, kinds


def kept_and_overwritten(before, after, groups):
    """(targets that kept every bit, targets that were overwritten), from a result alone"""
    kept = over = 0
    for t, _ in groups:
        same = all(np.array_equal(np.ascontiguousarray(before[f][t:t + 1]).view(np.uint32), np.ascontiguousarray(after[f][t:t + 1]).view(np.uint32))
                   for f in HANDED)
        kept, over = kept + same, over + (not same)
    return kept, over


def drop_every_second_writer(old):
    """the old map with match_id_forward = -1 on every second writer (in index order over all writers)"""
    old = old.copy()
    w = np.flatnonzero(old["match_id_forward"] >= 0)
    old["match_id_forward"][w[1::2]] = -1
    return old


# start velocities of minimizeVel and the accept masks the oracle gives for them on the stage's pair (iteration 0 is the last
# digit); the second and third are the second runs of section c
START_VELS = (((0.05, 0.0, 0.0), "00001"), ((0.0, 0.0, -0.06), "00001"), ((0.2, 0.1, 0.0), "01111"), ((0.0, 0.0, -0.9), "01111"))
RERUN_VELS = (START_VELS[1][0], START_VELS[2][0])


def targets_of(kl):
    f = kl["match_id_forward"]
    return set(f[f >= 0].tolist())


def behind_the_camera(kl, threshold, sigma_rho_min, vz):
    """keylines that tryVel evaluates (core.cpp:88-91) and that take its z_p <= 0 branch (core.cpp:96-98) at forward speed vz"""
    z_p = (1.0 / kl["rho"].astype(np.float64) + vz).astype(np.float32)
    return int(((kl["gradient_norm"] >= threshold) & (kl["sigma_rho"] <= sigma_rho_min) & (z_p <= 0)).sum())


DONOR = 936            # a well-matched keyline of the old map of the stage's pair (frames 3 -> 4)
DONOR_COPIES = 300     # old keylines 3, 9, 15, ... made copies of one well-matched donor
DONOR_FIELDS = ("pos", "pos_img", "gradient", "gradient_norm", "rho", "sigma_rho", "matches")


def craft_donor_copies(old, donor, varied):
    """Section e: DONOR_COPIES old keylines (3, 9, 15, ...) made copies of keyline `donor` in the fields tryVel reads, so that all
    of them forward to the donor's target through a whole pair. varied: rho * (1 + (k % 37 - 18) * 2^-14) on copy k - the
    maximum (k % 37 == 36) is shared by several copies."""
    old = old.copy()
    idx = 3 + 6 * np.arange(DONOR_COPIES)
    assert idx[-1] < len(old) and donor not in idx
    for f in DONOR_FIELDS:
        old[f][idx] = old[f][donor]
    if varied:
        k = np.arange(DONOR_COPIES)
        old["rho"][idx] = (old["rho"][donor] * (f32(1) + (k % 37 - 18).astype(np.float32) * f32(2.0 ** -14))).astype(np.float32)
        assert (old["rho"][idx] == old["rho"][idx].max()).sum() >= 2
    return old, idx


# ---- the oracle against the closed form ----------------------------------------------------------------------------------
def oracle_stage(orc_mod, stream):
    """The oracle's side of test_parity_gpu.warm(…, 3) and what the GPU file does next: three warm-up pairs, the keyline sums in
    the kernels' order from then on, the distance field of the fresh newest map. Returns (oracle, the three newest maps)."""
    frames, cam = stream
    orc = orc_mod.Oracle(params_for(orc_mod, cam, **KW))
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
    assert_bits_equal(o.keylines(), old, "the old map is read only")
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
    assert_bits_equal(got, want, "natural pair")
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
    assert_bits_equal(got, want, f"{layout}, {pattern}")
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
    assert_bits_equal(got, want, f"{layout}, {pattern}")
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
    assert_bits_equal(got, want, "second forwardMatch")
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


def assert_donor_pair(po, old_after, idx, varied):
    """Section e on the oracle's result alone: the pair tracks, one target has at least 257 writers from at least 2 workgroups
    (of 256 keylines, the smallest the kernels use), and the winner the crafted rhos call for."""
    assert po.status == 0, po.status
    t, m = max(writers_by_target(old_after).items(), key=lambda kv: len(kv[1]))
    assert len(m) >= 257 and len(np.unique(m // WG)) >= 2 and len(np.unique(m // 1024)) >= 2, (t, len(m))
    assert winner_of(old_after, m) == (1773 if varied else 1797)
    return t, m


@pytest.mark.parametrize("varied", [False, True], ids=["equal_rho", "varied_rho"])
def test_donor_copies_forward_to_one_target_through_a_pair(orc_mod, small_stream, varied):
    """Section e's precondition: with 300 old keylines made copies of keyline 936 the pair 3 -> 4 ends with status 0 and 1847
    matches, and all 301 forward to target 950, from 8 workgroups of 256."""
    frames, cam = small_stream
    orc = orc_mod.Oracle(params_for(orc_mod, cam, **KW))
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
