"""The oracle's per-keyline formulas against independent float64 statements of the same mathematics (CPU only).

The GPU parity tests compare the kernels with the oracle bit for bit, so the oracle's own arithmetic is what everything rests
on. Here the float64 statement is the reference and the fp32 oracle the code under test, as tests/test_fusion_math.py does
for the inertial fusion: the depth filter against a textbook scalar Kalman step (information form), searchMatch's probe range
against the reprojection of the keyline at rho and rho +- sigma_rho, regularize1Iter against the convex combination it is.

Each bar is four times the largest relative deviation measured over the keylines of the warmed 192x144 map, rounded up to one
digit (the factor covers another map); the measured value stands beside it. Keylines that the oracle clamps, resets or leaves
alone are compared exactly.
"""
import numpy as np
import pytest

from conftest import params_for
from support import KW_TRACK

RHO_MIN, RHO_MAX, RHO_INIT = 1e-3, 20.0, 1.0
RADIUS = 40.0


def _rel(got, want, floor=0.0):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) / np.maximum(np.abs(want), floor if floor else 1e-300)


@pytest.fixture(scope="module")
def stages(orc_mod, small_stream):
    """The pair after three warm-up pairs, stage by stage on the oracle: the newest map before directedMatch, after it, after
    regularize1Iter, after the depth filter; and what the stages were handed."""
    frames, cam = small_stream
    orc = orc_mod.Oracle(params_for(orc_mod, cam, **KW_TRACK))
    maps = [orc.detect_u8(frames[0], 0)]
    for i in range(1, 5):
        maps.append(orc.detect_u8(frames[i], i * 50000))
        if i < 4:
            orc.track_pair(maps[-2], maps[-1])
    old, new = maps[-2], maps[-1]
    orc.build_distance_field(new)
    ro = orc.minimize_vel(old)
    orc.forward_match(old, new)
    a = 0.0007
    Rb = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    out = dict(p=orc.p, orc=orc, V=ro["vel"].copy(), Rvel=ro["Rvel"].copy(), Rb=Rb, old=old.keylines(), before=new.keylines())
    n, _ = orc.directed_match(new, old, ro["vel"], ro["Rvel"], Rb, RADIUS)
    assert n > 1500
    out["matched"] = new.keylines()
    out["reg_num"] = orc.regularize(new)
    out["regularized"] = new.keylines()
    orc.update_inverse_depth(ro["vel"])
    out["filtered"] = new.keylines()
    return out


EKF_BAR = 2e-4     # measured 3.18e-5, 4 x 3.18e-5 = 1.27e-4 (the innovation Y - H rho_p cancels in fp32)


def test_depth_filter_is_a_scalar_kalman_step(stages):
    """Core::updateInverseDepthARLU (core.cpp:424-456). State rho, moved by the camera's forward motion: rho_p = rho / (1 + rho vz)
    with variance (d rho_p / d rho)^2 sigma^2 + q^2. Measurement: the displacement of the keyline along its match's unit
    gradient, Y = u . (q - q0), with the model Y = H rho, H = u . (v_xy fm - vz q0), and variance r^2. The update is written
    here in information form - 1 / P' = 1 / P_p + H^2 / r^2, rho' = P' (rho_p / P_p + H Y / r^2) - which is the same estimate
    as the gain form the reference evaluates, by other operations."""
    p, V = stages["p"], stages["V"].astype(np.float64)
    k0, k1 = stages["regularized"], stages["filtered"]
    m = k0["match_id"] >= 0
    same = ~m
    assert np.array_equal(k0["rho"][same].view(np.uint32), k1["rho"][same].view(np.uint32))
    assert np.array_equal(k0["sigma_rho"][same].view(np.uint32), k1["sigma_rho"][same].view(np.uint32))
    k0, k1 = k0[m], k1[m]
    fm, r, q_abs = float(p.fm), float(p.pixel_uncertainty), float(p.reshape_q_abs)
    rho, sig = k0["rho"].astype(np.float64), k0["sigma_rho"].astype(np.float64)
    u = k0["match_gradient"].astype(np.float64) / k0["match_gradient_norm"].astype(np.float64)[:, None]
    q, q0 = k0["pos_img"].astype(np.float64), k0["match_pos_img"].astype(np.float64)
    Y = np.einsum("ij,ij->i", u, q - q0)
    H = np.einsum("ij,ij->i", u, V[None, :2] * fm - V[2] * q0)
    rho_p = rho / (1.0 + rho * V[2])
    P_p = sig ** 2 / (1.0 + rho * V[2]) ** 4 + q_abs ** 2
    P_n = 1.0 / (1.0 / P_p + H ** 2 / r ** 2)
    rho_n = P_n * (rho_p / P_p + H * Y / r ** 2)
    sig_n = np.sqrt(P_n)
    lo, hi = rho_n < RHO_MIN, rho_n > RHO_MAX
    edge = (np.abs(rho_n - RHO_MIN) < 1e-5 * RHO_MIN) | (np.abs(rho_n - RHO_MAX) < 1e-5 * RHO_MAX)
    assert not edge.any()   # (no keyline of this map sits on a clamp: the classes below are unambiguous)
    assert (k1["rho"][lo] == np.float32(RHO_MIN)).all() and (k1["rho"][hi] == np.float32(RHO_MAX)).all()
    free = ~lo & ~hi
    assert free.sum() > 1500 and lo.sum() + hi.sum() >= 1
    assert not ((k1["rho"][free] == np.float32(RHO_INIT)) & (k1["sigma_rho"][free] == np.float32(RHO_MAX))).any()  # no reset
    # the clamp at kRhoMin hands the overshoot to sigma_rho (core.cpp:447-449)
    d_lo = _rel(k1["sigma_rho"][lo], sig_n[lo] + (RHO_MIN - rho_n[lo]))
    d = max(_rel(k1["rho"][free], rho_n[free]).max(), _rel(k1["sigma_rho"][free], sig_n[free]).max(), d_lo.max() if lo.any() else 0.0,
            _rel(k1["sigma_rho"][hi], sig_n[hi]).max() if hi.any() else 0.0)
    print(f"depth filter: largest relative deviation {d:.3g} over {int(m.sum())} keylines ({int(lo.sum())} at kRhoMin, {int(hi.sum())} at kRhoMax)")
    assert d <= EKF_BAR, d


SETUP_BAR = 2e-6   # measured 3.63e-7, 4 x 3.63e-7 = 1.45e-6


def test_search_range_is_the_reprojection_at_rho_and_rho_plus_minus_sigma(stages):
    """EdgeMap::searchMatch's probe range (edge_map.cpp:107-139). A point seen at pixel q (principal point at 0, rotated back) with
    inverse depth rho reprojects, to first order in the translation v, at q + rho J with J = -(v_xy fm - vz q): the search runs
    along J / |J|, expects the match at |J| rho and covers |J| (rho -+ sigma_rho), cut at 0 and at the radius and widened by the
    matching uncertainty; a keyline expected beyond the range is looked for from the middle of it. Deviations are relative to
    the value, or to one pixel where it is smaller."""
    p, orc = stages["p"], stages["orc"]
    Rb = stages["Rb"]
    Rb64 = Rb.astype(np.float64)
    fm, pu = float(p.fm), float(p.pixel_uncertainty_match)
    # the map's own keylines at the pair's velocity, and - for keylines expected beyond the range - the same with ten times the
    # inverse depth at a tenth of the uncertainty and eight times the velocity
    near = stages["before"].copy()
    near["rho"] = np.minimum(near["rho"] * np.float32(10.0), np.float32(RHO_MAX))
    near["sigma_rho"] *= np.float32(0.1)
    d, n_sure, n_beyond, n_within = 0.0, 0, 0, 0
    for kq, scale in ((stages["before"], 1.0), (near, 8.0)):
        vel_r32 = (Rb64 @ (scale * stages["V"].astype(np.float64))).astype(np.float32)
        got = orc.search_setup(kq, vel_r32, stages["Rvel"], Rb, RADIUS).astype(np.float64)
        v = vel_r32.astype(np.float64)
        ray = np.column_stack([kq["pos_img"].astype(np.float64), np.full(len(kq), fm)]) @ Rb64.T
        q = ray[:, :2] * (fm / ray[:, 2:3])
        rho = kq["rho"].astype(np.float64) * fm / ray[:, 2]
        sig = kq["sigma_rho"].astype(np.float64)
        J = -(v[None, :2] * fm - v[2] * q)
        nJ = np.linalg.norm(J, axis=1)
        assert (nJ > 1e-3).all()   # (the degenerate branch |t| <= 1e-6 is not what this map takes)
        lo = np.maximum(0.0, nJ * (rho - sig)) - pu
        hi = np.minimum(RADIUS, nJ * (rho + sig)) + pu
        mid = nJ * rho
        beyond = mid > hi
        sure = np.abs(mid - hi) > 1e-4
        mid = np.where(beyond, 0.5 * (lo + hi), mid)
        span = np.where(beyond, mid + 0.5, np.maximum(hi - mid, mid - lo))
        d = max(d, _rel(got[sure, 0], lo[sure], 1.0).max(), _rel(got[sure, 1], mid[sure], 1.0).max(),
                _rel(got[sure, 2], hi[sure], 1.0).max(), np.abs(got[:, 3:5] - J / nJ[:, None]).max(), _rel(got[:, 5], nJ).max())
        clear = sure & (span % 1.0 > 1e-3) & (span % 1.0 < 1 - 1e-3)    # (a truncation is only comparable away from the integers)
        assert np.array_equal(got[clear, 6], np.floor(span[clear])) and clear.sum() > 0.95 * len(kq)
        assert sure.sum() > 0.99 * len(kq)
        n_sure, n_beyond, n_within = n_sure + int(sure.sum()), n_beyond + int(beyond[sure].sum()), n_within + int((~beyond)[sure].sum())
    assert n_beyond >= 100 and n_within >= 100, (n_beyond, n_within)
    print(f"searchMatch range: largest relative deviation {d:.3g} over {n_sure} keylines ({n_beyond} expected beyond the range)")
    assert d <= SETUP_BAR, d


REG_BAR = 8e-7     # measured 1.91e-7, 4 x 1.91e-7 = 7.64e-7


def test_regularize_is_a_convex_combination_of_the_triple(stages):
    """EdgeMap::regularize1Iter (edge_map.cpp:220-259): a keyline whose two neighbours agree in depth within their uncertainty,
    (rho_n - rho_p)^2 <= sigma_n^2 + sigma_p^2, and in direction, cos(beta) >= threshold, takes the weighted mean of the triple -
    weights 1 / sigma^2 for itself and alpha / sigma^2 for each neighbour, alpha = (cos(beta) - thr) / (1 - thr) divided by
    1 + |rho_n - rho_p| / (sigma_n + sigma_p) - for rho and for sigma_rho alike. All from the values BEFORE the pass."""
    p = stages["p"]
    k0, k1 = stages["matched"], stages["regularized"]
    thr = float(p.regularization_threshold)
    both = (k0["id_prev"] >= 0) & (k0["id_next"] >= 0)
    c = np.flatnonzero(both)
    kn, kp = k0[k0["id_next"][c]], k0[k0["id_prev"][c]]
    f = lambda a: a.astype(np.float64)  # noqa: E731
    gap, room = (f(kn["rho"]) - f(kp["rho"])) ** 2, f(kn["sigma_rho"]) ** 2 + f(kp["sigma_rho"]) ** 2
    cosb = np.einsum("ij,ij->i", f(kn["gradient"]), f(kp["gradient"])) / (f(kn["gradient_norm"]) * f(kp["gradient_norm"]))
    takes = (gap <= room) & (cosb >= thr)
    sure = (np.abs(gap - room) > 1e-5 * room) & (np.abs(cosb - thr) > 1e-5)
    alpha = (cosb - thr) / (1.0 - thr) / (np.abs(f(kn["rho"]) - f(kp["rho"])) / (f(kn["sigma_rho"]) + f(kp["sigma_rho"])) + 1.0)
    w = np.stack([1.0 / f(k0["sigma_rho"][c]) ** 2, alpha / f(kn["sigma_rho"]) ** 2, alpha / f(kp["sigma_rho"]) ** 2])
    w /= w.sum(0)
    assert (w[:, takes] >= 0).all() and np.allclose(w.sum(0), 1.0)   # convex
    rho = w[0] * f(k0["rho"][c]) + w[1] * f(kn["rho"]) + w[2] * f(kp["rho"])
    sig = w[0] * f(k0["sigma_rho"][c]) + w[1] * f(kn["sigma_rho"]) + w[2] * f(kp["sigma_rho"])
    t, s = takes & sure, ~takes & sure
    assert t.sum() > 500 and s.sum() >= 10 and sure.sum() > 0.99 * len(c)
    # the count: every clear-cut triple that takes the mean, and at most the borderline ones besides
    assert int(t.sum()) <= stages["reg_num"] <= int(t.sum()) + int((~sure).sum()), (stages["reg_num"], int(t.sum()), int((~sure).sum()))
    # left alone: bit for bit what they were - the rejected triples and every keyline without two neighbours
    alone = np.concatenate([c[s], np.flatnonzero(~both)])
    for fld in ("rho", "sigma_rho"):
        assert np.array_equal(k0[fld][alone].view(np.uint32), k1[fld][alone].view(np.uint32)), fld
    d = max(_rel(k1["rho"][c[t]], rho[t]).max(), _rel(k1["sigma_rho"][c[t]], sig[t]).max())
    print(f"regularize1Iter: largest relative deviation {d:.3g} over {int(t.sum())} regularized keylines ({int(s.sum())} triples rejected)")
    assert d <= REG_BAR, d
