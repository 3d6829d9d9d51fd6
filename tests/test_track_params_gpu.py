"""GPU parity of the per-keyline tracking kernels away from the defaults: every parameter the kernels read from KParams moved
off the reference's default, long searches under a large pixel_uncertainty_match, crafted depth states that take every branch
of the depth filter and of regularize1Iter, and the corners of the sigma_rho quantile.

Every comparison is bit for bit against the CPU oracle (keyline sums in the kernels' order where sums are involved); this file
adds no tolerance. Everything runs on the 192x144 stream. A case that claims to reach a branch asserts that on the oracle's
result alone, before the library is looked at.
"""
import numpy as np
import pytest

from conftest import params_for
from support import B  # noqa: F401
from support import (KW_TRACK, RHO_MAX, RHO_MIN, Pair, assert_keylines_equal, assert_keylines_equal_nan, assert_pipeline_bit_identical, f32,
                     matching_stage, record_words, run_stream, set_forms, set_new_map)

pytestmark = pytest.mark.gpu

RHO_INIT = np.float32(1.0)  # types/keyline.hpp:15


def cvtt(x):
    return int(np.float32(x))  # truncation, as cvttss2si for the non-negative values here


def m3_mul(x, y):
    """the oracle's (and hostmath's) 3x3 product: fp32, s = 0, s += x[i][k] * y[k][j] in k order"""
    x, y = np.asarray(x, np.float32).reshape(3, 3), np.asarray(y, np.float32).reshape(3, -1)
    r = np.zeros((3, y.shape[1]), np.float32)
    for i in range(3):
        for j in range(y.shape[1]):
            s = np.float32(0)
            for k in range(3):
                s = np.float32(s + np.float32(x[i, k] * y[k, j]))
            r[i, j] = s
    return r


def rotate_inputs(vel, Rvel, Rb):
    """EdgeMap::directedMatch's prologue (edge_map.cpp:193-194): what searchMatch is handed"""
    Rb = np.asarray(Rb, np.float32)
    return m3_mul(Rb, np.asarray(vel, np.float32).reshape(3, 1)).reshape(3), m3_mul(m3_mul(Rb, Rvel), Rb.T.copy())


def small_rotation(a=0.0007):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)


# ---- 1. long searches ------------------------------------------------------------------------------------------------
def craft_long_searches(kl, p, vel_r, Rb, radius, pu):
    """Depths of the query keylines such that every search is long (edge_map.cpp:121-147): dq_rho = radius + 0.95 pu, just
    below dq_max = radius + pu, and sigma_rho = 1.5 rho, so dq_min = -pu and t_steps = cvtt(radius + 1.95 pu)."""
    kl = kl.copy()
    v = np.stack([kl["pos_img"][:, 0], kl["pos_img"][:, 1], np.full(len(kl), p.fm, np.float32)], 1).astype(np.float64)
    pm = v @ np.asarray(Rb, np.float64).T
    pmx, pmy = pm[:, 0] * p.fm / pm[:, 2], pm[:, 1] * p.fm / pm[:, 2]
    t_x, t_y = -(vel_r[0] * p.fm - vel_r[2] * pmx), -(vel_r[1] * p.fm - vel_r[2] * pmy)
    dq1 = np.hypot(t_x, t_y) * p.fm / pm[:, 2]      # dq_rho of rho = 1
    kl["rho"] = ((radius + 0.95 * pu) / dq1).astype(np.float32)
    kl["sigma_rho"] = np.float32(1.5) * kl["rho"]
    return kl


# velocity handed to directedMatch, in units of the pair's minimizeVel result. The reversed sign puts real edges at t in
# [-pu, -2), which only the far end of the descending chain reaches; the scale is chosen per pu so that enough of the oracle's
# matches are accepted there (counts in the test's docstring)
LONG_VEL_SCALE = -3.0
# radius of the search: the reference's 40, but 40.5 at pu = 3 - with an integer radius R and pu = 3 the longest search of this
# recipe has cvtt(R + 1.95 pu) = R + 5 steps, which is exactly where the kernel used to stop (cvtt(R + pu) + 2); half a pixel
# more makes it R + 6
LONG_RADIUS = {0: 40.0, 1: 40.0, 3: 40.5, 5: 40.0, 8: 40.0}


@pytest.mark.parametrize("head", [None, "compact4", "compact1"], ids=["compact8", "compact4", "compact1"])
@pytest.mark.parametrize("pu", [0, 1, 3, 5, 8])
def test_long_searches_under_pixel_uncertainty_match(orc_mod, B, small_stream, monkeypatch, pu, head):
    """Phase 2 of k_directed_match_c used to stop its long searches at cvtt(max_radius + pu) + 2 steps while search_setup asks for
    up to cvtt(max_radius + 2 pu): for pu > 2 the far end of the descending chain was dropped, in all three forms of the kernel
    (8 / 4 / 1 lanes per keyline), while the single-keyline entry walked every step. Here every search of the newest map is
    crafted long (craft_long_searches) and directedMatch is handed -3 times the pair's velocity, so that real edges lie at
    t in [-pu, -2). On the oracle (2015 keylines, step = the probe step at which the match is accepted):
      pu 0: 248 matches; pu 1: 283; pu 3 (radius 40.5): 637, 60 of them at a step >= 45; pu 5: 927, 44 at a step >= 47;
      pu 8: 1730, 146 at a step >= 50.
    For pu >= 3 at least 20 such matches are required of the oracle before the library is looked at; with the old bound these
    cases fail (directedMatch's count and match fields differ) for pu 3, 5 and 8 in every form. Then: counts and every keyline
    field of directedMatch, the single-keyline entry on 200 evenly spaced keylines, regularize1Iter and the depth filter."""
    set_forms(monkeypatch, head=head)
    radius = LONG_RADIUS[pu]
    P, ro = matching_stage(orc_mod, B, small_stream, pixel_uncertainty_match=float(pu))
    om_old, om_new = P.om
    gm_old, gm_new = P.gm
    Rb = small_rotation()
    V = (np.float32(LONG_VEL_SCALE) * ro["vel"]).astype(np.float32)
    vel_r, Rvel_r = rotate_inputs(V, ro["Rvel"], Rb)
    kl = craft_long_searches(om_new.keylines(), P.orc.p, vel_r, Rb, radius, pu)
    assert kl["rho"].min() >= RHO_MIN and kl["rho"].max() <= RHO_MAX, (kl["rho"].min(), kl["rho"].max())
    set_new_map(P, kl)
    # the oracle alone: which old keyline every search accepts, and at which step of the probe loop
    ids, steps = P.orc.search_match_steps(om_old, kl, vel_r, Rvel_r, Rb, radius)
    late = int((steps >= cvtt(radius + pu) + 2).sum())
    print(f"pu {pu}: {int((ids >= 0).sum())} matches of {len(kl)}, {late} accepted at a step >= {cvtt(radius + pu) + 2}, "
          f"longest accepted step {steps.max()}")
    if pu >= 3:
        assert late >= 20, late
    no, kfo = P.orc.directed_match(om_new, om_old, V, ro["Rvel"], Rb, max_radius=radius)
    ko = om_new.keylines()
    assert no == int((ids >= 0).sum()) and np.array_equal(ko["match_id"][ids >= 0], ids[ids >= 0])
    assert no > 200
    ng, kfg = P.ctx.directed_match(gm_new, gm_old, V, ro["Rvel"], Rb, max_radius=radius)
    assert (no, kfo) == (ng, kfg)
    assert_keylines_equal(ko, gm_new.keylines(), what=f"directedMatch, pu {pu}")
    for i in np.linspace(0, len(kl) - 1, 200).astype(int):
        got = gm_old.search_match(kl[i], vel_r, Rvel_r, Rb, max_radius=radius)
        assert got == ids[i], (i, got, ids[i], steps[i])
    ro_n, rg_n = P.orc.regularize(om_new), P.ctx.regularize(gm_new)
    assert ro_n == rg_n
    assert_keylines_equal(om_new.keylines(), gm_new.keylines(), what=f"regularize, pu {pu}")
    P.orc.update_inverse_depth(V)
    P.ctx.update_inverse_depth(V)
    assert_keylines_equal_nan(om_new.keylines(), gm_new.keylines(), what=f"depth EKF, pu {pu}")


def test_directed_match_refuses_a_radius_beyond_the_probe_buffer(orc_mod, B, small_stream):
    """rebvio_hip_directed_match bounds max_radius + 2 * pixel_uncertainty_match like rebvio_hip_create bounds search_range:
    with pu = 8 a radius of 242 is the last one accepted (242 + 16 + 2 = 260), 243 is refused although it is below 255."""
    P, ro = matching_stage(orc_mod, B, small_stream, n_warm=1, pixel_uncertainty_match=8.0)
    Rb = small_rotation()
    with pytest.raises(B.HipError, match="pixel_uncertainty_match"):
        P.ctx.directed_match(P.gm[1], P.gm[0], ro["vel"], ro["Rvel"], Rb, max_radius=243.0)
    with pytest.raises(B.HipError, match="max_radius"):
        P.ctx.directed_match(P.gm[1], P.gm[0], ro["vel"], ro["Rvel"], Rb, max_radius=256.0)
    no, kfo = P.orc.directed_match(P.om[1], P.om[0], ro["vel"], ro["Rvel"], Rb, max_radius=242.0)
    ng, kfg = P.ctx.directed_match(P.gm[1], P.gm[0], ro["vel"], ro["Rvel"], Rb, max_radius=242.0)
    assert (no, kfo) == (ng, kfg) and no > 100
    assert_keylines_equal(P.om[1].keylines(), P.gm[1].keylines(), what="directedMatch, radius 242, pu 8")


# ---- 2. matching gates -----------------------------------------------------------------------------------------------
def gate_stage(O, B, stream, **kw):
    P, ro = matching_stage(O, B, stream, **kw)
    Rb = small_rotation()
    radius = float(P.orc.p.search_range)
    no, kfo = P.orc.directed_match(P.om[1], P.om[0], ro["vel"], ro["Rvel"], Rb, max_radius=radius)
    return P, ro, Rb, radius, no, kfo


@pytest.fixture(scope="module")
def default_gate_count(orc_mod, B, small_stream):
    return gate_stage(orc_mod, B, small_stream)[4]


GATES = ([dict(match_threshold_angle=a) for a in (5.0, 45.0, 90.0, 180.0)] +
         [dict(match_threshold_norm=v) for v in (0.05, 1.0, 10.0)] +
         [dict(search_range=r, pixel_uncertainty_match=u) for r in (8.0, 40.0, 120.0) for u in (0.0, 8.0)])
GATE_DEFAULTS = (dict(match_threshold_angle=45.0), dict(match_threshold_norm=1.0))


@pytest.mark.parametrize("kw", GATES, ids=lambda kw: ",".join(f"{k}={v:g}" for k, v in kw.items()))
def test_matching_gates(orc_mod, B, small_stream, default_gate_count, kw):
    """The gates of searchMatch (edge_map.cpp:166-177) and the search radius away from their defaults, at the pair's own
    velocity: directedMatch counts and every keyline field, then regularize1Iter and the depth filter on the result. Each
    non-default value moves the oracle's match count off the default's, so a kernel with the default as a literal cannot pass."""
    P, ro, Rb, radius, no, kfo = gate_stage(orc_mod, B, small_stream, **kw)
    print(f"{kw}: {no} matches, default {default_gate_count}")
    if kw not in GATE_DEFAULTS:
        assert no != default_gate_count, (kw, no)
    else:
        assert no == default_gate_count
    assert no > 100
    ng, kfg = P.ctx.directed_match(P.gm[1], P.gm[0], ro["vel"], ro["Rvel"], Rb, max_radius=radius)
    assert (no, kfo) == (ng, kfg)
    assert_keylines_equal(P.om[1].keylines(), P.gm[1].keylines(), what=f"directedMatch {kw}")
    assert P.orc.regularize(P.om[1]) == P.ctx.regularize(P.gm[1])
    assert_keylines_equal(P.om[1].keylines(), P.gm[1].keylines(), what=f"regularize {kw}")
    P.orc.update_inverse_depth(ro["vel"])
    P.ctx.update_inverse_depth(ro["vel"])
    assert_keylines_equal_nan(P.om[1].keylines(), P.gm[1].keylines(), what=f"depth EKF {kw}")


# ---- 3. one parameter at a time through the whole pipeline ------------------------------------------------------------
GYRO_STD, GYRO_BIAS_STD = 1.6968e-04, 1.9393e-05   # the reference's defaults (types/imu.hpp)
ONE_PARAM = ([dict(reweight_distance=v) for v in (0.5, 8.0)] +
             [dict(match_treshold=v) for v in (0.1, 2.0)] +
             [dict(min_match_threshold=v) for v in (1, 10000)] +
             [dict(pixel_uncertainty=v) for v in (0.25, 4.0)] +
             [dict(reshape_q_abs=v) for v in (0.0, 0.1)] +
             [dict(regularization_threshold=v) for v in (0.0, 0.9)] +
             [dict(quantile_cutoff=v) for v in (0.5, 0.99)] +
             [dict(quantile_num_bins=v) for v in (1, 2, 63, 127, 128)] +
             [dict(iterations=v) for v in (1, 2, 9)] +
             [dict(gyro_std_dev=GYRO_STD * s) for s in (10.0, 0.1)] +
             [dict(gyro_bias_std_dev=GYRO_BIAS_STD * s) for s in (10.0, 0.1)] +
             [dict(cx_off=17.5, cy_off=-11.25), dict(fm_scale=0.7), dict(pixel_uncertainty_match=8.0)])
COMBINED = dict(reweight_distance=0.5, match_treshold=2.0, min_match_threshold=1, pixel_uncertainty=0.25, reshape_q_abs=0.1,
                regularization_threshold=0.9, quantile_cutoff=0.5, quantile_num_bins=63, iterations=2,
                gyro_std_dev=GYRO_STD * 10.0, gyro_bias_std_dev=GYRO_BIAS_STD * 0.1, cx_off=17.5, cy_off=-11.25, fm_scale=0.7,
                pixel_uncertainty_match=8.0)
N_FRAMES = 6


def pipeline_kw(cam, over):
    """parameter overrides of a case: the camera entries are given relative to the stream's camera"""
    kw = dict(KW_TRACK)
    for k, v in over.items():
        if k == "cx_off":
            kw["cx"] = cam.cx + v
        elif k == "cy_off":
            kw["cy"] = cam.cy + v
        elif k == "fm_scale":
            kw["fm"] = cam.fm * v
        else:
            kw[k] = v
    return kw


def oracle_run(O, frames, cam, kw, n=N_FRAMES):
    """the oracle alone over the first n frames: (words of the last pair record, newest map, pair statuses, last klm_num)"""
    orc = O.Oracle(params_for(O, cam, **kw))
    orc.set_sum_order("device")
    maps, status = [], []
    for k in range(n):
        maps.append(orc.detect_u8(frames[k], k * 50000))
        if k:
            po = orc.track_pair(maps[-2], maps[-1])
            status.append(po.status)
    return record_words(po), maps[-1].keylines(), status, po.klm_num


@pytest.fixture(scope="module")
def default_run(orc_mod, small_stream):
    frames, cam = small_stream
    return oracle_run(orc_mod, frames, cam, dict(KW_TRACK))


def moved_off_default(run, default_run):
    w, kl, _, _ = run
    w0, kl0, _, _ = default_run
    if not np.array_equal(w, w0) or len(kl) != len(kl0):
        return True
    return any(not np.array_equal(kl[f], kl0[f]) for f in kl.dtype.names)


def ids_of(over):
    return ",".join(f"{k}={v:g}" for k, v in over.items())


@pytest.mark.parametrize("over", ONE_PARAM, ids=ids_of)
def test_pipeline_with_one_parameter_moved(orc_mod, B, small_stream, default_run, over):
    """Six frames through the per-pair API and through the streaming driver (device glue), state carried independently on both
    sides, with ONE parameter off its default: every word of every pair record and every field of the newest map. The oracle's
    last record or newest map differs from the default run's, so the parameter is live in the pipeline."""
    frames, cam = small_stream
    kw = pipeline_kw(cam, over)
    run = oracle_run(orc_mod, frames, cam, kw)
    if "min_match_threshold" in over:
        # Core::tryVel gates on min(min_match_threshold, frame_count_) and the reference never advances frame_count_
        # (core.cpp:22, :91), so no value of this parameter can move anything: the cases stay, with the opposite precondition
        assert not moved_off_default(run, default_run), over
    else:
        assert moved_off_default(run, default_run), over
    assert run[2] == [0] * (N_FRAMES - 1), run[2]
    assert_pipeline_bit_identical(orc_mod, B, frames, cam, list(range(N_FRAMES)), kw, 100, what=ids_of(over), every_pair_tracks=True)


def test_pipeline_with_every_parameter_moved(orc_mod, B, small_stream, default_run):
    """All of them off their defaults at once (one value each)."""
    frames, cam = small_stream
    kw = pipeline_kw(cam, COMBINED)
    run = oracle_run(orc_mod, frames, cam, kw)
    assert moved_off_default(run, default_run)
    assert_pipeline_bit_identical(orc_mod, B, frames, cam, list(range(N_FRAMES)), kw, 100, what="combined", every_pair_tracks=True)


def test_batch_lanes_equal_stand_alone_streams_with_every_parameter_moved(B, small_stream):
    """Two lanes of a batch (the batch form of every tracking kernel) at the combined setting: each lane's records, word for
    word, are those of a stand-alone streaming context on the same frames."""
    from rebvio_amd import synth
    frames, cam = small_stream
    kw = pipeline_kw(cam, COMBINED)
    streams = [frames, synth.render_stream(cam.width, cam.height, len(frames), stream_id=1)[0]]
    npx = cam.width * cam.height
    order = list(range(N_FRAMES))
    alone = []
    for s in streams:
        ctx = B.Context(params_for(B, cam, **kw))
        dev = ctx.upload_frames(s)
        alone.append([(record_words(o), n) for o, n in run_stream(ctx, dev, order, npx)])
        ctx.close()
    bat = B.Batch(params_for(B, cam, **kw), 2)
    devs = [bat.lanes[s].upload_frames(streams[s]) for s in range(2)]
    got = [[], []]
    for k, i in enumerate(order):
        outs, nks = bat.push_u8_device([d + i * npx for d in devs], k * 50000)
        for s in range(2):
            if outs[s].status >= 0:
                got[s].append((record_words(outs[s]), nks[s]))
    for outs, nks in bat.flush():
        for s in range(2):
            got[s].append((record_words(outs[s]), nks[s]))
    bat.close()
    for s in range(2):
        assert len(got[s]) == len(alone[s]) == N_FRAMES - 1
        assert alone[s][-1][0][-1] == 0, "the last pair of the stand-alone stream tracks"   # status word
        for k, ((wa, na), (wb, nb)) in enumerate(zip(alone[s], got[s])):
            assert na == nb and np.array_equal(wa, wb), (s, k, np.flatnonzero(wa != wb)[:8])


# ---- 4. crafted depth states -----------------------------------------------------------------------------------------


def one_ulp_pair(rp, sn, sp):
    """rn >= rp, adjacent fp32 values (pass, fail): (rn - rp)^2 > sn^2 + sp^2 is false for the first and true for the next one
    up, every operation in fp32 as regularize1Iter evaluates it (edge_map.cpp:234)"""
    rp, sn, sp = f32(rp), f32(sn), f32(sp)
    rhs = f32(f32(sn * sn) + f32(sp * sp))

    def over(rn):
        d = f32(rn - rp)
        return f32(d * d) > rhs
    rn = f32(rp + np.sqrt(rhs))
    while over(rn):
        rn = np.nextafter(rn, f32(-np.inf), dtype=np.float32)
    while not over(np.nextafter(rn, f32(np.inf), dtype=np.float32)):
        rn = np.nextafter(rn, f32(np.inf), dtype=np.float32)
    return rn, np.nextafter(rn, f32(np.inf), dtype=np.float32)


def craft_triples(kl, thr, scale=1.0, unmatchable=False, alpha_at=True):
    """120 hand-made triples (centre, id_prev, id_next) on keylines that have both neighbours, no keyline used twice; returns
    dict name -> centre keylines. scale: a power of two on the triples' gradients and norms (alpha is their ratio: unchanged, and
    exact). unmatchable: the triples' keylines are taken out of every match - pos_img far outside the image, so that searchMatch
    probes nothing for them, and, with a small `scale`, a gradient that fails Core::testfk against every real keyline, so that
    forwardMatch hands them nothing either - and keep the depths crafted here until regularize1Iter reads them. alpha_at=False
    puts the 'alpha exactly at the threshold' triples one ulp below it instead (the control of a count comparison)."""
    s = f32(scale)
    inner = np.flatnonzero((kl["id_prev"] >= 0) & (kl["id_next"] >= 0))
    used = set()
    picks = []
    for c in inner:   # (no keyline next to two triples either: every other triple of the map keeps its natural neighbours)
        t = (int(c), int(kl["id_prev"][c]), int(kl["id_next"][c]))
        halo = set(t) | {int(kl[f][j]) for j in t for f in ("id_prev", "id_next")}
        if len(set(t)) == 3 and not used & halo:
            used |= halo
            picks.append(t)
    assert len(picks) >= 120, len(picks)
    made = dict(sigma_apart=[], ulp_pass=[], ulp_fail=[], alpha_at=[], alpha_below=[])
    below = np.nextafter(f32(thr), f32(-1), dtype=np.float32)
    for k, (c, ip, inx) in enumerate(picks[:120]):
        kind = k % 5
        # a well-behaved triple to start from: gradients parallel, depths close
        for j in (c, ip, inx):
            kl["gradient"][j] = (3.0 * s, 4.0 * s)
            kl["gradient_norm"][j] = 5.0 * s
            kl["rho"][j] = 1.5
            kl["sigma_rho"][j] = 0.25
            if unmatchable:
                kl["pos_img"][j] = (1e4, 1e4)
        if kind == 0:    # neighbours' sigma_rho 1e-3 against 20
            kl["sigma_rho"][inx], kl["sigma_rho"][ip] = RHO_MIN, RHO_MAX
            kl["rho"][inx], kl["rho"][ip] = 1.5 + 0.125 * (k % 7), 1.25
            made["sigma_apart"].append(c)
        elif kind in (1, 2):  # the depth-gap test one ulp either side
            rp = f32(1.0 + 0.25 * (k % 3))
            if (k // 5) % 2 == 0:   # the gap EQUAL to the room, (5/8)^2 = (3/8)^2 + (4/8)^2 with every term exact: > and >= part here
                sn, sp = f32(0.375), f32(0.5)
                ok = f32(rp + f32(0.625))
                fail = np.nextafter(ok, f32(np.inf), dtype=np.float32)
                assert f32(ok - rp) == f32(0.625) and f32(0.625) * f32(0.625) == f32(sn * sn) + f32(sp * sp)
            else:
                sn, sp = f32(0.25 + 0.03125 * (k % 11)), f32(0.125 + 0.0625 * (k % 5))
                ok, fail = one_ulp_pair(rp, sn, sp)
            kl["sigma_rho"][inx], kl["sigma_rho"][ip] = sn, sp
            kl["rho"][ip], kl["rho"][inx] = rp, (ok if kind == 1 else fail)
            made["ulp_pass" if kind == 1 else "ulp_fail"].append(c)
        else:            # alpha exactly at the threshold / one ulp below: neighbours of norm `scale` whose cosine is thr
            kl["gradient"][inx], kl["gradient_norm"][inx] = (s, 0.0), s
            a = f32(thr) if kind == 3 and alpha_at else below
            kl["gradient"][ip], kl["gradient_norm"][ip] = (a * s, 0.75 * s), s
            made["alpha_at" if kind == 3 else "alpha_below"].append(c)
    return {k: np.array(v) for k, v in made.items()}


def cycle_depths(kl):
    """rho and sigma_rho cycled through {kRhoMin, kRhoMax, natural}, all nine combinations"""
    i = np.arange(len(kl))
    kl["rho"] = np.where(i % 3 == 0, RHO_MIN, np.where(i % 3 == 1, RHO_MAX, kl["rho"]))
    kl["sigma_rho"] = np.where((i // 3) % 3 == 0, RHO_MIN, np.where((i // 3) % 3 == 1, RHO_MAX, kl["sigma_rho"]))


def craft_depth_states(kl, thr, alpha_at=True):
    """The newest map after directedMatch, with depth states that natural data does not produce. Returns the crafted array and
    the indices of the hand-made triples: dict name -> centre keylines."""
    kl = kl.copy()
    cycle_depths(kl)
    # 0 / 0 in the depth filter's unit gradient on every 7th keyline
    kl["match_gradient"][::7] = 0
    kl["match_gradient_norm"][::7] = 0
    return kl, craft_triples(kl, thr, alpha_at=alpha_at)


def bits_changed(a, b):
    return (a["rho"].view(np.uint32) != b["rho"].view(np.uint32)) | (a["sigma_rho"].view(np.uint32) != b["sigma_rho"].view(np.uint32))


def assert_triples_on_oracle(made, changed):
    """what regularize1Iter did to the centres of the hand-made triples, from the oracle's result alone"""
    assert changed[made["ulp_pass"]].all() and not changed[made["ulp_fail"]].any()
    assert not changed[made["alpha_below"]].any()
    assert changed[made["sigma_apart"]].any()


DEPTH_VEL = {"natural": None, "vz=-1/rho": (0.0, 0.0, -1.0 / 20.0)}


@pytest.mark.parametrize("thr", [0.5, 0.0], ids=["thr0.5", "thr0"])
@pytest.mark.parametrize("vel_kind", list(DEPTH_VEL))
def test_crafted_depth_states_through_regularize_and_depth_filter(orc_mod, B, small_stream, vel_kind, thr):
    """k_regularize and k_depth_ekf on a map crafted after directedMatch (craft_depth_states): rho and sigma_rho cycled through
    {kRhoMin, kRhoMax, natural}, a 0 / 0 unit gradient on every 7th keyline, and 120 hand-made triples - neighbours' sigma_rho
    1e-3 against 20, the depth-gap test passed and failed by one ulp of rho (half of them with the gap EQUAL to the room), alpha exactly at the regularization threshold and
    one ulp below it - at the pair's own velocity and at (0, 0, -1/20), which sends every keyline at kRhoMax through 1 / 0.
    On the oracle: 1039 (threshold 0.5) / 1090 (threshold 0) of 1943 keylines with two neighbours are regularized; after the
    filter, natural velocity: 8 at kRhoMin, 158 at kRhoMax, 284 reset to (1, 20), 0-1 sigma_rho > 20; vz = -1/20: 328 at kRhoMin,
    58 at kRhoMax, 510 reset, 15 sigma_rho > 20 and 3 sigma_rho left NaN beside a rho clamped from +inf (core.cpp:450 comes before
    the NaN test), which is why the comparison takes a NaN for a NaN. A triple with alpha AT the threshold is regularized with
    weight zero, which leaves its centre as it was: that it is taken shows in the count alone, which is 24 higher than on a copy
    of the map with those 24 triples one ulp below the threshold."""
    P, ro = matching_stage(orc_mod, B, small_stream, regularization_threshold=thr)
    om_old, om_new = P.om
    gm_old, gm_new = P.gm
    Rb = small_rotation()
    no, kfo = P.orc.directed_match(om_new, om_old, ro["vel"], ro["Rvel"], Rb)
    assert P.ctx.directed_match(gm_new, gm_old, ro["vel"], ro["Rvel"], Rb) == (no, kfo)
    matched = om_new.keylines()
    kl, made = craft_depth_states(matched, thr)
    set_new_map(P, kl)
    V = ro["vel"] if DEPTH_VEL[vel_kind] is None else np.array(DEPTH_VEL[vel_kind], np.float32)
    # the oracle alone
    control = om_new.clone()
    control.set_keylines(craft_depth_states(matched, thr, alpha_at=False)[0])
    reg_n = P.orc.regularize(om_new)
    assert reg_n - P.orc.regularize(control) == len(made["alpha_at"]) == 24
    kr = om_new.keylines()
    inner = (kl["id_prev"] >= 0) & (kl["id_next"] >= 0)
    assert reg_n >= 50 and int(inner.sum()) - reg_n >= 50, (reg_n, int(inner.sum()))
    assert_triples_on_oracle(made, bits_changed(kr, kl))
    P.orc.update_inverse_depth(V)
    ke = om_new.keylines()
    m = ke["match_id"] >= 0
    at_min = int((m & (ke["rho"] == RHO_MIN)).sum())
    at_max = int((m & (ke["rho"] == RHO_MAX)).sum())
    reset = int((m & (ke["rho"] == RHO_INIT) & (ke["sigma_rho"] == RHO_MAX) & ~((kr["rho"] == RHO_INIT) & (kr["sigma_rho"] == RHO_MAX))).sum())
    wide = int((ke["sigma_rho"] > RHO_MAX).sum())
    nans = int(np.isnan(ke["rho"]).sum() + np.isnan(ke["sigma_rho"]).sum())
    print(f"{vel_kind}, thr {thr}: regularized {reg_n} of {int(inner.sum())} with both neighbours; after the filter {at_min} at kRhoMin, "
          f"{at_max} at kRhoMax, {reset} reset, {wide} sigma_rho > 20, {nans} NaN")
    assert at_max >= 20 and reset >= 20, (at_max, reset)
    if vel_kind != "natural":  # (at the pair's own velocity few depths leave the range downwards: 8 here)
        assert at_min >= 20 and wide >= 1, (at_min, wide)
    # the library on the same array
    assert P.ctx.regularize(gm_new) == reg_n
    assert_keylines_equal_nan(kr, gm_new.keylines(), what="regularize, crafted")
    P.ctx.update_inverse_depth(V)
    assert_keylines_equal_nan(ke, gm_new.keylines(), what="depth EKF, crafted")


def craft_pair_maps(kl_old, kl_new, thr, alpha_at=True):
    """Both maps of a pair, crafted BEFORE the pair so that the fused regularize_ekf_body meets the states above.
    Older map: depths cycled - directedMatch hands them to the newest map's matches (edge_map.cpp:203-204) - and on every 7th
    keyline a zero gradient with sigma_rho = kRhoMax: tryVel passes such a keyline over (gradient_norm below the map's threshold,
    core.cpp:90), searchMatch's gates let it through (its cosine is NaN, its norm ratio is 0: neither comparison rejects), so its
    match inherits a 0 / 0 unit gradient and the filter has to reset it.
    Newest map: the 120 triples, unmatchable (craft_triples), so regularize1Iter reads them as crafted."""
    old, new = kl_old.copy(), kl_new.copy()
    cycle_depths(old)
    old["gradient"][::7] = 0
    old["gradient_norm"][::7] = 0
    old["sigma_rho"][::7] = RHO_MAX
    made = craft_triples(new, thr, scale=2.0 ** -20, unmatchable=True, alpha_at=alpha_at)
    return old, new, made


def test_crafted_depth_states_through_whole_pairs(orc_mod, B, small_stream):
    """The fused regularize_ekf_body - regularize1Iter + depth filter + the histogram of the next pair's quantile, the copy that
    track_pair, the streaming driver and the batch run - on the crafted states, through whole pairs (craft_pair_maps). On the
    oracle's result alone, before the library runs: the pair tracks (status 0); of the newest map's matched keylines at least 20
    end at kRhoMin, 20 at kRhoMax and 20 reset to (1, 20) behind a zero match_gradient, one sigma_rho exceeds 20; at least 50
    keylines are regularized and 50 with two neighbours left alone; the centres of the one-ulp triples changed where the gap test
    passes and kept their bits where it fails, those one ulp below the alpha threshold kept theirs; and the 24 triples AT the
    threshold are counted: a second oracle driven over the same frames with those triples one ulp below reports 24 fewer.
    Then every word of the pair record and every field of the newest map; then one more pair, whose sigma_rho_min comes from
    the bins of the fused kernel. Counts on the oracle: 1456 matches, 1245 of 1943 regularized (control 1221), 55 at kRhoMin,
    350 at kRhoMax, 257 reset behind a zero gradient, 14 sigma_rho > 20, no NaN left."""
    frames, cam = small_stream
    thr = 0.5
    P = Pair(orc_mod, B, frames, cam, **KW_TRACK)
    P.orc.set_sum_order("device")
    ctl = orc_mod.Oracle(params_for(orc_mod, cam, **KW_TRACK))   # the control of the alpha count
    ctl.set_sum_order("device")
    cm = [ctl.detect_u8(frames[0], 0)]
    P.detect(0)
    for i in (1, 2, 3, 4):   # (all sides track: the gyro-bias filter carries state from pair to pair)
        P.detect(i)
        cm = [cm[-1], ctl.detect_u8(frames[i], i * 50000)]
        if i < 4:
            P.orc.track_pair(P.om[0], P.om[1])
            P.ctx.track_pair(P.gm[0], P.gm[1])
            ctl.track_pair(cm[0], cm[1])
    assert_keylines_equal(P.om[0].keylines(), cm[0].keylines(), what="control oracle")
    old, new, made = craft_pair_maps(P.om[0].keylines(), P.om[1].keylines(), thr)
    P.om[0].set_keylines(old)
    set_new_map(P, new)
    P.sync_gpu_from_oracle()
    old_c, new_c, _ = craft_pair_maps(cm[0].keylines(), cm[1].keylines(), thr, alpha_at=False)
    cm[0].set_keylines(old_c)
    cm[1].set_keylines(new_c)
    po = P.orc.track_pair(P.om[0], P.om[1])
    pc = ctl.track_pair(cm[0], cm[1])
    ko = P.om[1].keylines()
    m = ko["match_id"] >= 0
    at_min, at_max = int((m & (ko["rho"] == RHO_MIN)).sum()), int((m & (ko["rho"] == RHO_MAX)).sum())
    reset = int((m & (ko["match_gradient_norm"] == 0) & (ko["rho"] == RHO_INIT) & (ko["sigma_rho"] == RHO_MAX)).sum())
    wide = int((ko["sigma_rho"] > RHO_MAX).sum())
    inner = int(((ko["id_prev"] >= 0) & (ko["id_next"] >= 0)).sum())
    nans = int(np.isnan(ko["rho"]).sum() + np.isnan(ko["sigma_rho"]).sum())
    print(f"pair on crafted maps: status {po.status}, {po.klm_num} matches, {po.reg_num} of {inner} regularized (control {pc.reg_num}), "
          f"{at_min} at kRhoMin, {at_max} at kRhoMax, {reset} reset behind a zero gradient, {wide} sigma_rho > 20, {nans} NaN")
    assert po.status == 0 and pc.status == 0
    assert at_min >= 20 and at_max >= 20 and reset >= 20 and wide >= 1, (at_min, at_max, reset, wide)
    assert po.reg_num >= 50 and inner - po.reg_num >= 50
    triple = np.concatenate(list(made.values()))
    assert (ko["match_id"][triple] == -1).all()    # (unmatched: the depth filter left what regularize1Iter wrote)
    assert_triples_on_oracle(made, bits_changed(ko, new))
    assert po.reg_num - pc.reg_num == len(made["alpha_at"]) == 24, (po.reg_num, pc.reg_num)
    # the library
    pg = P.ctx.track_pair(P.gm[0], P.gm[1])
    assert np.array_equal(record_words(po), record_words(pg)), np.flatnonzero(record_words(po) != record_words(pg))[:8]
    assert_keylines_equal_nan(ko, P.gm[1].keylines(), what="newest map after the pair on crafted maps")
    # the next pair starts from the histogram the fused kernel has binned
    P.detect(5)
    po2 = P.orc.track_pair(P.om[0], P.om[1])
    pg2 = P.ctx.track_pair(P.gm[0], P.gm[1])
    assert po2.status == 0
    assert f32(po2.sigma_rho_min).view(np.uint32) == f32(pg2.sigma_rho_min).view(np.uint32), (po2.sigma_rho_min, pg2.sigma_rho_min)
    assert np.array_equal(record_words(po2), record_words(pg2))
    assert_keylines_equal_nan(P.om[1].keylines(), P.gm[1].keylines(), what="newest map after the following pair")


QUANTILE_CORNERS = ("last_bin", "bin0", "outside")


def craft_sigma(kl, corner):
    kl = kl.copy()
    if corner == "last_bin":
        kl["sigma_rho"] = RHO_MAX
    elif corner == "bin0":
        kl["sigma_rho"] = RHO_MIN
    else:  # beyond both ends: clamped into the end bins (edge_map.cpp:43-45)
        kl["sigma_rho"] = np.where(np.arange(len(kl)) % 2 == 0, f32(25.0), f32(1e-4))
    return kl


def expected_quantile(corner, bins, pct, n):
    """estimateQuantile (edge_map.cpp:39-56) on the crafted histograms, from its definition: the lower edge of the first bin
    before which MORE than pct * n keylines lie, 1e3 when there is none"""
    counts = np.zeros(bins, np.int64)
    if corner == "last_bin":
        counts[bins - 1] = n
    elif corner == "bin0":
        counts[0] = n
    else:
        counts[bins - 1] += (n + 1) // 2
        counts[0] += n // 2
    before = np.concatenate([[0], np.cumsum(counts)[:-1]])
    hit = np.flatnonzero(before.astype(np.float32) > f32(pct) * f32(n))
    if not len(hit):
        return f32(1e3)
    return f32(f32(f32(hit[0]) * f32(RHO_MAX - RHO_MIN)) / f32(bins) + RHO_MIN)


@pytest.mark.parametrize("pct", [0.0, 0.9, 1.0])
@pytest.mark.parametrize("bins", [1, 127, 128])
@pytest.mark.parametrize("corner", QUANTILE_CORNERS)
def test_quantile_corners(orc_mod, B, small_stream, corner, bins, pct):
    """estimateQuantile (edge_map.cpp:39-56) where its loop ends: every sigma_rho in the last bin (no bin has MORE than pct * n
    keylines before it: 1e3), every one in bin 0, and values beyond both ends of [kRhoMin, kRhoMax], which are clamped into the
    end bins - with 1, 127 and 128 bins (two per lane in the wave form, the odd count leaves the last lane half empty) and
    pct 0, 0.9 and 1. The expected value is worked out from the definition; the oracle is held to it first, then the stand-alone
    entry (a lone lane's loop) and the sigma_rho_min of a pair (the wave form at the head of the LM kernel)."""
    frames, cam = small_stream
    P = Pair(orc_mod, B, frames, cam, **dict(KW_TRACK, quantile_cutoff=pct, quantile_num_bins=bins))
    P.orc.set_sum_order("device")
    P.detect(0)
    P.detect(1)
    P.orc.track_pair(P.om[0], P.om[1])
    P.ctx.track_pair(P.gm[0], P.gm[1])
    P.detect(2)
    kl = craft_sigma(P.om[0].keylines(), corner)
    P.om[0].set_keylines(kl)
    P.sync_gpu_from_oracle()
    want = expected_quantile(corner, bins, pct, len(kl))
    qo = f32(P.orc.quantile(P.om[0], pct, bins))
    assert qo.view(np.uint32) == want.view(np.uint32), (qo, want)
    qg = f32(P.ctx.quantile(P.gm[0], pct, bins))
    assert qg.view(np.uint32) == qo.view(np.uint32), (qg, qo)
    po = P.orc.track_pair(P.om[0], P.om[1])
    assert f32(po.sigma_rho_min).view(np.uint32) == want.view(np.uint32), (po.sigma_rho_min, want)
    pg = P.ctx.track_pair(P.gm[0], P.gm[1])
    assert np.array_equal(record_words(po), record_words(pg)), (po.sigma_rho_min, pg.sigma_rho_min, po.status, pg.status)
    assert_keylines_equal_nan(P.om[1].keylines(), P.gm[1].keylines(), what=f"newest map, {corner} {bins} {pct}")
