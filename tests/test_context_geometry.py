"""The entries that go through kfp::lookup (rebvio_amd/csrc/kf_pose.hpp) away from the default context, without a GPU: the rows of
tests/context_cases.py - a ragged 131x67 frame with a quarter-pixel principal point, EuRoC's intrinsics over four, a principal point
near a corner, search_range 3, 7, 100 and 255 - through the host hooks that run the kernels' source (rebvio_hip_test_kf_align_host,
_align_many_host, _fuse_host, _handover_host) on the oracle's frame of each row:
  - the owner identity of tests/test_keyframe_lookup.py: alignment, fusion and hand-over associate the same keylines with the same
    owners, and that mask is the restatement's - with all six exits of the lookup planted and taken, and per side of the frame a
    keyline in the outermost column / row that nothing but the border test keeps out;
  - one evaluation against np_kf_align_sums at the crafted motion and at a seeded guess: assoc element for element, the 28 sums within
    (used + 64) * 2^-52 * sum |term| (the bar of tests/test_keyframe_align.py); three guesses through the many-hypothesis hook equal
    the single hook byte for byte (the bar of tests/test_keyframe_align_many.py);
  - the fusion's and the hand-over's records, matches, assoc words and counts against np_kf_fuse and np_kf_handover, every word
    (the bars of tests/test_keyframe_fuse.py and tests/test_keyframe_handover.py).
The hooks take the field as ids and distances, so the device's key decode is not in this half (tests/test_context_geometry_gpu.py);
fm, the principal point, the border test against cols - 2 / rows - 2 and the cell index y * cols + x are. A camera read as
(cols / 2, rows / 2) turns rows A, B and C red here and leaves D, whose camera is the synthetic one, green.

Non-vacuity is a condition of every row and is asserted on the restatement before anything is compared (context_cases.host_case)."""
import numpy as np
import pytest

from context_cases import CONTEXTS, IDS, host_case, host_scene
from kf_align_many_ref import seeded_guesses
from kf_align_ref import GUARD, LOOKUP_EXITS, np_kf_align_sums
from kf_fuse_ref import INT_MIN, np_kf_fuse, perturbed
from kf_fuse_ref import counts_of as fuse_counts
from kf_handover_ref import assert_identities, guard_min, np_kf_handover, purpose_case
from kf_handover_ref import counts_of as handover_counts
from kf_pose_ref import pose_sums, true_motion
from support import F32
from support import backend  # noqa: F401


def crafted_data(sc, prs4=None, normals=True):
    c = sc["craft"]
    return (sc["cam"], c["prs4"] if prs4 is None else prs4, c["kf_matches"], c["normals"] if normals else None, sc["pos"], sc["unit"], sc["ids"],
            sc["dists"])


@pytest.mark.parametrize("cid", IDS)
def test_the_rows_are_what_they_claim(orc_mod, cid):
    """the scene of each row: the oracle's camera is the row's, the frame is the row's, the field reaches search_range, and - C, D -
    past what the default range reaches"""
    c = CONTEXTS[cid]
    sc = host_scene(orc_mod, cid)
    fm, cx, cy, rows, cols = sc["cam"]
    assert (rows, cols) == (c["height"], c["width"]) and len(sc["ids"]) == rows * cols
    assert (F32(fm), F32(cx), F32(cy)) == (F32(c["fm"]), F32(c["cx"]), F32(c["cy"]))
    assert cid == "D" or (cx != cols / 2 and cy != rows / 2)      # (D keeps the synthetic camera: its row is about df_nr alone)
    owned = sc["ids"] >= 0
    far = int(sc["dists"][owned].max())
    sr = int(c["search_range"])
    print(f"{cid}: {len(sc['kl'])} keylines, {len(sc['craft']['prs4'])} crafted, {owned.mean():.3f} of the cells owned, farthest at {far}")
    assert len(sc["kl"]) > 500 and len(sc["craft"]["prs4"]) > 0.9 * len(sc["kl"])
    assert far <= sr and (far == sr if sr <= 7 else far > 40)
    # the oracle's field in D holds cells at the distance the max_dist plant chose in the issue's run, 152, at least: bit 7 of the
    # key's 9-bit distance field is needed from 128 on
    assert cid != "D" or far >= 152


@pytest.mark.parametrize("cid", IDS)
def test_alignment_fusion_and_handover_find_the_same_owners(backend, orc_mod, cid):
    B = backend
    sc, case, want = host_case(orc_mod, cid)
    assert set(case["plants"]) == set(LOOKUP_EXITS)
    n = len(case["prs4"])
    print(f"{cid}: {n} keyframe keylines, {int(want.sum())} associated, max_dist {case['max_dist']}, plants {case['plants']}")
    R, t = true_motion()
    args = (*sc["cam"], sc["search_range"], case["prs4"], case["kf_matches"], case["normals"], case["pos"], case["unit"], case["ids"],
            case["dists"])
    md = dict(max_dist=case["max_dist"])
    _, align = B.kf_align_host(*args, B.default_kf_align_opts(max_iter=0, **md), R, t)
    _, _, _, fuse = B.kf_fuse_host(*args, B.default_kf_fuse_opts(**md), R, t)
    dst = np.zeros((len(case["pos"]), 4), F32)
    dst[:, 2:] = (1.0, 0.5)
    _, _, _, handover = B.kf_handover_host(*args, dst, np.ones(len(dst), np.uint32), B.default_kf_handover_opts(**md), R, t)
    a_has, f_has, h_has = align >= 0, fuse != INT_MIN, handover != INT_MIN
    assert np.array_equal(a_has, f_has) and np.array_equal(a_has, h_has), (np.flatnonzero(a_has != f_has)[:8], np.flatnonzero(a_has != h_has)[:8])
    owner = lambda x: np.where(x >= 0, x, -1 - x.astype(np.int64))
    assert np.array_equal(owner(fuse)[a_has], align[a_has]) and np.array_equal(owner(handover)[a_has], align[a_has])
    assert np.array_equal(a_has, want), np.flatnonzero(a_has != want)[:8]
    # every planted exit is one the hooks take, and of the rim plants (context_cases.rim_plants) the outer one is dropped and its
    # control in the next column / row kept: `cols - 1` for `cols - 2` in the border test would keep the plant of x = cols - 1
    assert not a_has[[j for name, j in case["plants"].items()]].any()
    assert case["sides"] and all(not a_has[case["rim"][s]] for s in case["sides"])
    assert all(a_has[j] for name, j in case["rim"].items() if name not in case["sides"])


def host_evaluation(B, sc, d, R, t, what, **opts):
    """assert_evaluation of tests/test_keyframe_align.py: one evaluation on both sides at (R, t)"""
    S, absS, used, assoc, g = np_kf_align_sums(*d, R, t, **opts)
    assert min(g.values()) > GUARD, (what, g)
    got, a = B.kf_align_host(*d[0], sc["search_range"], *d[1:], B.default_kf_align_opts(max_iter=0, **opts), R, t)
    assert np.array_equal(a, assoc), (what, np.flatnonzero(a != assoc)[:8], a[a != assoc][:8], assoc[a != assoc][:8])
    assert got.used == used and got.candidates == len(d[1]) and got.iterations == 0, (what, got.used, used)
    diff = np.abs(pose_sums(got) - S)
    bound = (used + 64) * 2.0 ** -52 * absS
    assert (diff <= bound).all(), (what, np.flatnonzero(diff > bound))
    return used, got


@pytest.mark.parametrize("cid", IDS)
def test_one_evaluation_against_the_restatement(backend, orc_mod, cid):
    sc = host_scene(orc_mod, cid)
    d = crafted_data(sc)
    sr = dict(max_dist=sc["search_range"])
    R, t = true_motion()
    used, _ = host_evaluation(backend, sc, d, R, t, f"{cid}: crafted motion", **sr)
    assert used >= 0.99 * len(d[1]), (used, len(d[1]))
    (Rg, tg), = seeded_guesses(1, 11, R, t)
    used_g, _ = host_evaluation(backend, sc, d, Rg, tg, f"{cid}: seeded guess", **sr)
    assert 12 <= used_g <= len(d[1])
    print(f"{cid}: used {used} at the crafted motion, {used_g} at the seeded guess, of {len(d[1])}")


@pytest.mark.parametrize("cid", IDS)
def test_many_hypotheses_equal_the_single_hook_byte_for_byte(backend, orc_mod, cid):
    B = backend
    sc = host_scene(orc_mod, cid)
    d = crafted_data(sc)
    R, t = true_motion()
    guesses = [(R, t)] + seeded_guesses(2, 12, R, t)
    for max_iter in (0, 8):
        opts = B.default_kf_align_opts(max_iter=max_iter, max_dist=sc["search_range"])
        res = B.kf_align_many_host(*d[0], sc["search_range"], *d[1:], [g[0] for g in guesses], [g[1] for g in guesses], opts)
        assert len(res) == 3
        for k, ((R0, t0), r) in enumerate(zip(guesses, res)):
            one, _ = B.kf_align_host(*d[0], sc["search_range"], *d[1:], opts, R0, t0)
            assert bytes(r.pose) == bytes(one), (cid, max_iter, k, r.pose.status, one.status, r.pose.used, one.used)
            assert 0 <= r.inliers <= r.pose.used and r.pose.used >= 12


@pytest.mark.parametrize("cid", IDS)
def test_fusion_against_the_restatement_bit_for_bit(backend, orc_mod, cid):
    B = backend
    sc = host_scene(orc_mod, cid)
    R, t = true_motion()
    prs4, _ = perturbed(sc["craft"], 11)
    d = crafted_data(sc, prs4)
    for what, kw in (("the context's reach", dict(max_dist=sc["search_range"])),
                     ("no gradient test, short reach, tight gate", dict(min_cos=-1.0, max_dist=1, gate_sigma=0.8, q_abs=0.02, pixel_sigma=0.5))):
        ref = np_kf_fuse(*d, R, t, **kw)
        assert min(ref["guards"].values()) > GUARD, (cid, what, ref["guards"])
        out, p, mt, assoc = B.kf_fuse_host(*d[0], sc["search_range"], *d[1:], B.default_kf_fuse_opts(**kw), R, t)
        print(f"{cid}, {what}: {fuse_counts(ref)}")
        assert fuse_counts(out) == fuse_counts(ref), (cid, what, fuse_counts(out), fuse_counts(ref))
        assert np.array_equal(assoc, ref["assoc"]), (cid, what, np.flatnonzero(assoc != ref["assoc"])[:8])
        assert p.tobytes() == ref["prs4"].tobytes(), (cid, what, np.flatnonzero((p != ref["prs4"]).any(1))[:8])
        assert np.array_equal(mt, ref["matches"]), (cid, what)
        assert out.associated == out.fused + out.gated + out.flat
        assert ref["fused"] > 0.5 * len(prs4), (cid, what, fuse_counts(ref))


@pytest.mark.parametrize("cid", IDS)
def test_handover_against_the_restatement_bit_for_bit(backend, orc_mod, cid):
    B = backend
    sc = host_scene(orc_mod, cid)
    R, t = true_motion()
    P = purpose_case(sc, 1)
    d = (sc["cam"], P["src_prs4"], P["src_matches"], P["src_normals"], sc["pos"], sc["unit"], sc["ids"], sc["dists"], P["dst_prs4"], P["dst_matches"])
    for what, kw in (("the context's reach", dict(max_dist=sc["search_range"])),
                     ("no gradient test, short reach, tight gate", dict(min_cos=-1.0, max_dist=1, gate_sigma=0.8, q_abs=0.02))):
        ref = np_kf_handover(*d, R, t, **kw)
        assert guard_min(ref) > GUARD, (cid, what, ref["guards"])
        out, p, mt, assoc = B.kf_handover_host(*d[0], sc["search_range"], *d[1:], B.default_kf_handover_opts(**kw), R, t)
        print(f"{cid}, {what}: {handover_counts(ref)}")
        assert handover_counts(out) == handover_counts(ref), (cid, what, handover_counts(out), handover_counts(ref))
        assert np.array_equal(assoc, ref["assoc"]), (cid, what, np.flatnonzero(assoc != ref["assoc"])[:8])
        assert p.tobytes() == ref["prs4"].tobytes(), (cid, what, np.flatnonzero((p != ref["prs4"]).any(1))[:8])
        assert np.array_equal(mt, ref["matches"]), (cid, what)
        assert_identities(handover_counts(out))
        assert ref["adopted"] > 0.3 * len(P["src_prs4"]), (cid, what, handover_counts(ref))


def test_the_hooks_follow_the_range_they_are_given(backend, orc_mod):
    """max_dist = search_range is accepted and search_range + 1 refused with -3, naming max_dist, at 3 and at 255; without opts the
    reach is the range handed over"""
    B = backend
    for cid in ("B", "D"):
        sc = host_scene(orc_mod, cid)
        sr = sc["search_range"]
        assert sr == int(CONTEXTS[cid]["search_range"])
        d = crafted_data(sc)
        R, t = true_motion()
        args = (*d[0], sr, *d[1:])
        dst = np.zeros((len(sc["pos"]), 4), F32)
        dst[:, 2:] = (1.0, 0.5)
        dm = np.ones(len(dst), np.uint32)
        calls = ((B.kf_align_host, args, B.default_kf_align_opts), (B.kf_fuse_host, args, B.default_kf_fuse_opts),
                 (B.kf_handover_host, (*args, dst, dm), B.default_kf_handover_opts))
        for fn, a, mk in calls:
            fn(*a, mk(max_dist=sr), R, t)
            with pytest.raises(B.HipError) as e:
                fn(*a, mk(max_dist=sr + 1), R, t)
            assert "error -3:" in str(e.value) and "max_dist" in str(e.value), (cid, fn.__name__, str(e.value))
        # opts = None: max_dist is the range handed to the hook
        none, a_none = B.kf_align_host(*args, None, R, t)
        full, a_full = B.kf_align_host(*args, B.default_kf_align_opts(max_dist=sr), R, t)
        assert bytes(none) == bytes(full) and np.array_equal(a_none, a_full)


def test_a_fractional_search_range_reaches_one_step_further_on_the_oracle(orc_mod):
    """Why rebvio_hip_create refuses a fractional search_range (tests/test_abi.py): the reference walks
    `for (int r = -search_range_; r < search_range_; ++r)` with the float as the upper bound (core.hpp:49), and so does the oracle -
    at 7.5 r runs over -7 .. 7, at 7.0 over -7 .. 6 - while the device's kernels walk [-(df_nr >> 1), df_nr >> 1) with
    df_nr = 2 * (int)search_range and would build the 7.0 field for both. On frame 2 of the 160x120 synthetic stream (fm 114.5,
    cx 80, cy 60; the same keylines under both ranges) the two fields differ, and every differing cell is one the 7.5 field owns at
    distance 7: the step r = +7. Counts of this run: 450 of 19 200 cells differ; 13 449 cells are owned at 7.5 against 12 999 at 7.0."""
    from rebvio_amd import synth
    frames, cam = synth.render_stream(160, 120, 3)
    assert (cam.fm, cam.cx, cam.cy) == (114.5, 80.0, 60.0)
    fields, kls = [], []
    for sr in (7.0, 7.5):
        orc = orc_mod.Oracle(orc_mod.default_params(120, 160, fm=cam.fm, cx=cam.cx, cy=cam.cy, search_range=sr))
        for k in range(3):
            m = orc.detect_u8(frames[k], k * 50000)
        orc.build_distance_field(m)
        fields.append(orc.distance_field())
        kls.append(m.keylines())
    assert kls[0].tobytes() == kls[1].tobytes() and len(kls[0]) > 1000      # one detected map
    (ids7, d7), (ids75, d75) = fields
    differ = (ids7 != ids75) | (d7 != d75)
    print(f"{int(differ.sum())} of {differ.size} cells differ; owned: {int((ids75 >= 0).sum())} at 7.5, {int((ids7 >= 0).sum())} at 7.0")
    assert differ.sum() > 0
    assert (ids75[differ] >= 0).all() and (d75[differ] == 7).all()
    assert (int(differ.sum()), int((ids75 >= 0).sum()), int((ids7 >= 0).sum())) == (450, 13449, 12999)
