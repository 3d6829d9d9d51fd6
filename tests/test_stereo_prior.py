"""The stereo prior without a device: the ABI surface and its argument checks, the host hook (rebvio_hip_test_stereo_prior_host: the
statements of rebvio_amd/csrc/stereo_prior.hpp, which the kernel runs too) against the numpy restatement of the header's definition
(tests/stereo_prior_ref.py) bit for bit, planted cases worked out by hand (tests/stereo_prior_cases.py), and what the prior buys on
the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import stereo_prior_cases as SC
import stereo_prior_ref as R
from conftest import params_for
from support import KW_TRACK, backend  # noqa: F401

F32 = np.float32
# Statistic A of test_value_on_the_oracle as measured with this restatement on the 192x144 stereo stream; the bound on
# it is twice this and absorbs nothing but changes of the synthetic scene.
A_MEASURED = 0.009390
BASELINE = 0.2


def both(B, rows, cols, fm, left, right, mask, **opts):
    """the hook and the restatement on the same input, asserted equal in every word; -> (counts tuple, keylines, outcome, winner)"""
    c, k2, oc, win = B.stereo_prior_host(rows, cols, fm, left, right, mask, B.default_stereo_prior_opts(**opts))
    c2, k3, oc2, win2 = R.stereo_prior(left, right, mask, rows, cols, fm, **opts)
    assert c.as_tuple() == R.counts_tuple(c2), (c.as_tuple(), R.counts_tuple(c2))
    assert np.array_equal(oc, oc2), np.flatnonzero(oc != oc2)[:8]
    assert np.array_equal(win, win2), np.flatnonzero(win != win2)[:8]
    for f in left.dtype.names:
        a, b = k2[f].view(np.uint32), k3[f].view(np.uint32)
        assert np.array_equal(a, b), (f, np.flatnonzero((a != b).reshape(len(left), -1).any(1))[:8])
    for f in left.dtype.names:  # nothing but rho and sigma_rho moves
        if f not in ("rho", "sigma_rho"):
            assert np.array_equal(k2[f].view(np.uint32), np.ascontiguousarray(left[f]).view(np.uint32)), f
    still = (oc & 7) != 1
    assert np.array_equal(k2["rho"][still].view(np.uint32), left["rho"][still].view(np.uint32))
    assert np.array_equal(k2["sigma_rho"][still].view(np.uint32), left["sigma_rho"][still].view(np.uint32))
    assert np.array_equal(win >= 0, ~still) and (win < max(len(right), 1)).all()
    n_oc = np.bincount(oc & 7, minlength=5)
    assert c.candidates == len(left) and c.usable == len(left) - n_oc[3] and c.seen == c.fused + c.gated + c.ambiguous
    assert (c.fused, c.gated, c.ambiguous, c.clamped, c.reserved) == (n_oc[1], n_oc[2], n_oc[4], int((oc & 32 != 0).sum()), 0)
    return c.as_tuple(), k2, oc, win


@pytest.fixture(scope="module")
def stereo_run(orc_mod):
    """the 192x144 stereo stream (10 frames, baseline 0.2) on the CPU oracle with the restatement's fusion, computed once"""
    from rebvio_amd import synth
    left, right, cam = synth.render_stereo_stream(192, 144, 10, BASELINE)
    depth = synth.render_stream_depth(cam.width, cam.height, 10)
    p = params_for(orc_mod, cam, **KW_TRACK)
    return left, right, cam, depth, p, R.oracle_stream(orc_mod, p, left, right, BASELINE, depth)


# ---- the ABI surface --------------------------------------------------------------------------------------------------------------
def test_defaults_and_layout(backend):
    B = backend
    o = B.default_stereo_prior_opts()
    assert (o.baseline, o.d_min, o.d_max, o.min_ux, o.row_tol, o.sigma_px, o.gate_sigma, o.ambig_px, o.norm_tol, o.q_abs, o.reserved) == \
        (0.0, 0.0, 64.0, 0.5, 1, 0.5, 3.0, 2.0, 1.0, 0.0, 0)
    assert o.cos_min == R.COS45 and abs(o.cos_min - np.cos(np.pi / 4)) < 1e-7
    assert C.sizeof(B.StereoPriorOpts) == 96 and C.sizeof(B.StereoPriorCounts) == 32
    assert {k: getattr(o, k) for k in R.DEFAULTS} == R.DEFAULTS


def test_left_frames_are_render_streams(backend):
    from rebvio_amd import synth
    left, right, cam = synth.render_stereo_stream(96, 72, 2, 0.1)
    mono, cam2 = synth.render_stream(96, 72, 2)
    assert np.array_equal(left, mono) and cam == cam2
    assert right.shape == left.shape and not np.array_equal(left, right)
    again = synth.render_stereo_stream(96, 72, 2, 0.1)[1]
    assert np.array_equal(right, again)
    # the partner at baseline 0 sees the left view, under noise of its own
    same = synth.render_stereo_stream(96, 72, 1, 0.0, noise=False)
    assert np.array_equal(same[0], same[1])


BAD_OPTS = (dict(baseline=0.0), dict(baseline=-0.1), dict(baseline=float("nan")), dict(baseline=float("inf")), dict(d_min=-1.0),
            dict(d_min=float("nan")), dict(d_min=65.0), dict(d_max=97.0), dict(d_max=float("nan")), dict(min_ux=0.0), dict(min_ux=1.5),
            dict(min_ux=float("nan")), dict(row_tol=2), dict(row_tol=-1), dict(sigma_px=0.0), dict(sigma_px=float("nan")),
            dict(sigma_px=float("inf")), dict(gate_sigma=0.0), dict(gate_sigma=float("nan")), dict(ambig_px=-1.0),
            dict(ambig_px=float("nan")), dict(cos_min=1.5), dict(cos_min=float("nan")), dict(norm_tol=-1.0), dict(norm_tol=float("nan")),
            dict(q_abs=-1.0), dict(q_abs=float("nan")), dict(reserved=1))


def test_every_refusal_is_minus_3_before_a_device_is_touched(backend):
    B = backend
    L = B.lib()
    rows, cols = SC.ROWS, SC.COLS
    kl = SC.keylines(4)
    kl["pos"] = (40.0, 5.0)
    kr, mask = SC.plant(rows, cols, [SC.at(35.0, 5.0)])
    cnt = B.StereoPriorCounts()
    good = B.default_stereo_prior_opts(baseline=SC.BASE)

    def hook(rows=rows, cols=cols, k=kl, n=4, r=kr, nr=1, m=mask, opts=good, counts=cnt):
        return L.rebvio_hip_test_stereo_prior_host(rows, cols, SC.FM, k.ctypes.data if k is not None else None, n,
                                                   r.ctypes.data if r is not None else None, nr, m.ctypes.data if m is not None else None,
                                                   opts, C.byref(counts) if counts is not None else None, None, None)
    assert hook() == 0 and cnt.fused == 4
    assert hook(opts=None) == -3  # the defaults hold no baseline
    assert L.rebvio_hip_last_error().decode().startswith("test_stereo_prior_host: baseline")
    for kw in BAD_OPTS:
        assert hook(opts=B.default_stereo_prior_opts(**dict(dict(baseline=SC.BASE), **kw))) == -3, kw
        assert L.rebvio_hip_last_error().decode().startswith("test_stereo_prior_host"), kw
    assert hook(opts=B.default_stereo_prior_opts(baseline=SC.BASE, d_max=float(cols))) == 0  # d_max = cols is the last one accepted
    assert hook(k=None) == -3 and hook(r=None) == -3 and hook(m=None) == -3 and hook(counts=None) == -3
    assert hook(n=-1) == -3 and hook(nr=-1) == -3 and hook(rows=-1) == -3 and hook(cols=-1) == -3
    assert hook(k=None, n=0) == 0 and hook(r=None, nr=0) == 0
    # the device entries refuse a null handle before anything else
    assert L.rebvio_hip_map_fuse_stereo(None, None, good, C.byref(cnt), None, None) == -3
    assert L.rebvio_hip_map_fuse_stereo_async(None, None, None, good) == -3
    assert L.rebvio_hip_stereo_prior_last_counts(None, C.byref(cnt)) == -3


# ---- the hook against the restatement -----------------------------------------------------------------------------------------------
def test_hook_equals_restatement_on_the_oracles_stereo_stream(backend, stereo_run):
    _, _, cam, _, _, run = stereo_run
    total = np.zeros(8, np.int64)
    for k in range(len(run["before"])):
        kr, mask = run["right"][k]
        c, k2, oc, _ = both(backend, cam.height, cam.width, cam.fm, run["before"][k], kr, mask, baseline=BASELINE)
        assert c == R.counts_tuple(run["counts"][k]) and np.array_equal(oc, run["outcomes"][k])
        assert np.array_equal(k2["rho"].view(np.uint32), run["keylines"][k]["rho"].view(np.uint32))
        total += c
    assert (total[1:6] > 0).all(), total


def test_hook_equals_restatement_on_200_random_tables(backend, stereo_run):
    _, _, cam, _, _, run = stereo_run
    rng = np.random.default_rng(21)
    seen = np.zeros(8, np.int64)
    kinds = np.zeros(5, np.int64)
    for it in range(200):
        if it % 2:
            rows, cols, fm = cam.height, cam.width, cam.fm
            kr, mask = run["right"][it % len(run["right"])]  # a detected right map
            base = BASELINE
        else:
            rows, cols, fm, base = 33, 37, SC.FM, SC.BASE
            kr, mask = SC.random_right_map(rng, rows, cols, int(rng.integers(0, 400)))
        opts = dict(baseline=base, d_max=min(64.0, float(cols)))
        if it % 5 == 0:
            lo = float(rng.uniform(0, 10))
            opts.update(d_min=lo, d_max=min(lo + float(rng.uniform(0, 25)), float(cols)), row_tol=int(rng.integers(0, 2)), min_ux=float(rng.uniform(0.1, 1.0)),
                        ambig_px=float(rng.uniform(0, 4)), q_abs=float(rng.uniform(0, 1)), sigma_px=float(rng.uniform(0.1, 2)),
                        cos_min=float(rng.uniform(0, 1)), norm_tol=float(rng.uniform(0, 2)))
        kl = SC.left_from_right(rng, kr, rows, cols, int(rng.integers(0, 300)), fm * base, d_hi=30.0)
        c, _, oc, _ = both(backend, rows, cols, fm, kl, kr, mask, **opts)
        seen += c
        kinds += np.bincount(oc & 7, minlength=5)
    assert (kinds > 300).all(), kinds  # every outcome occurs in numbers
    assert seen[6] > 0, seen


# ---- planted cases, outcomes worked out by hand -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.planted_cases(), ids=lambda c: c[0])
def test_planted(backend, case):
    name, rows, cols, fm, left, right, mask, opts, want, want_win = case
    c, k2, oc, win = both(backend, rows, cols, fm, left, right, mask, **opts)
    assert list(oc) == want, (name, list(oc))
    if want_win is not None:
        assert list(win) == want_win, (name, list(win))
    if name == "gate":  # K = 0: the fused ones keep their value
        assert np.array_equal(k2["rho"].view(np.uint32), left["rho"].view(np.uint32)) and list(k2["sigma_rho"]) == [0.0, 0.0, 0.0]
    if name == "tie":   # keyline 0 takes d = 5 of j = 0 (rho_m = 0.5), not d = 6 of j = 1
        s_m = 0.05
        K = 400.0 / (400.0 + s_m * s_m)
        assert abs(float(k2["rho"][0]) - (1.0 + K * (0.5 - 1.0))) < 1e-6 and abs(float(k2["sigma_rho"][0]) - s_m) < 1e-6
    if name == "clamp_high":
        assert k2["rho"][0] == F32(20.0)
    if name == "clamp_low":
        assert k2["rho"][0] == F32(1e-3) and abs(float(k2["sigma_rho"][0]) - (5e-5 + (1e-3 - 5e-4))) < 1e-6  # the overshoot goes to sigma_rho
    if name == "sigma_zero":
        assert list(k2["rho"]) == [F32(0.5), F32(0.6)] and list(k2["sigma_rho"]) == [0.0, 0.0]
    if name == "sigma_zero_q_abs":
        assert abs(float(k2["rho"][1]) - 0.5) < 1e-4


def test_fresh_keylines_take_the_metric_depth(backend):
    """z = fm * baseline / d: 2 m and 4 m at fb = 10 are d = 5 and d = 2.5"""
    B = backend
    kl = SC.keylines(2)
    kl["pos"] = ((40.0, 5.0), (40.0, 15.0))
    kr, mask = SC.plant(SC.ROWS, SC.COLS, [SC.at(35.0, 5.0), SC.at(37.5, 15.0)])
    c, k2, oc, win = both(B, SC.ROWS, SC.COLS, SC.FM, kl, kr, mask, baseline=SC.BASE)
    assert list(oc) == [1, 1] and list(win) == [0, 1]
    assert abs(1.0 / float(k2["rho"][0]) - 2.0) < 1e-3 and abs(1.0 / float(k2["rho"][1]) - 4.0) < 1e-3
    assert np.allclose(k2["sigma_rho"], 0.05, rtol=1e-4) and np.array_equal(k2["matches"], kl["matches"])


# ---- what it buys -------------------------------------------------------------------------------------------------------------------
def test_value_on_the_oracle(orc_mod, stereo_run):
    """The 192x144 KW_TRACK stream, 10 frames, on the CPU oracle in device sum order; the right view is rendered 0.2 m along the
    camera's x axis with noise of its own, detected by a second oracle, and fused by the restatement into map k after its pair (map
    0: after detection). A = the median over frames 2..9 of the median relative depth error |1 / rho - z| / z of the
    default-cloud-filter keylines against the rendered depth, taken before that frame's own fusion; B = the same without stereo.
    Measured: A = 0.009390, B = 0.5633; |V| 0.0194 - 0.0218 against the scene's 0.0229 m per frame (0.0139 - 0.0146, scale-free,
    without stereo); 1344 - 1789 keylines pass the filter against 809 - 1482."""
    left, right, cam, depth, p, a = stereo_run
    b = R.oracle_stream(orc_mod, p, left, None, BASELINE, depth)
    A, Bv = float(np.median(a["err"][2:])), float(np.median(b["err"][2:]))
    v_a = [float(np.linalg.norm(r.V)) for r in a["records"]]
    v_b = [float(np.linalg.norm(r.V)) for r in b["records"]]
    print(f"A = {A:.6f}  B = {Bv:.6f}  |V| with stereo {min(v_a):.4f}..{max(v_a):.4f}  without {min(v_b):.4f}..{max(v_b):.4f}  "
          f"passing {a['passing'][2:]} against {b['passing'][2:]}")
    for c in a["counts"]:
        print(R.counts_tuple(c))
    assert all(r.status == 0 for r in a["records"]) and all(r.status == 0 for r in b["records"])
    assert A <= Bv / 10, (A, Bv)
    assert A <= 2 * A_MEASURED, (A, A_MEASURED)
    for kind in range(5):  # every outcome occurs in at least one frame
        assert any((oc & 7 == kind).any() for oc in a["outcomes"]), kind
