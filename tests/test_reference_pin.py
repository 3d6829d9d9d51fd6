"""The oracle against the reference's own hot-path code, compiled: oracle/_ref/librebvio_ref.so (scale_space.cpp, edge_detector.cpp,
edge_map.cpp and core.cpp of the reference checkout, unmodified, behind oracle/ref_driver.cpp and the stand-in headers of
oracle/ref_shim/). The reference library gives the expected value, oracle/rebvio_oracle.cpp is the code under test, in its default
(reference) sum order. Everything is compared as 32-bit words (support.bits_equal / support.words: a float by its bits, a NaN is a
NaN); the one exception is the solution X of extRotVel, see test_ext_rot_vel.

Inputs: the 192x144 small_stream with KW_TRACK; for the detection stages also 32x32 and 33x35, the smallest and an odd-width size
of test_envelope_gpu's grid (uniform noise frames, which is what that file's frames are at these sizes).

One process serves every case: the reference keeps the detector's plane-fit pseudo-inverse in a function-local static, but
plane_fit_size is a compile-time constant of the reference (edge_detector.hpp) - orc_params has no such field and the settings of
test_detect_params_gpu cannot change it - and the other function-local statics (the Ls4 and mean-acceleration histories) belong to
glue that no case here calls. So no case needs a second value of such a static and none runs in a child process.

Of the inertial glue one function is compared: Core::gyroBiasCorrection (core.cpp:264-284; public, no static state) gives the
expected X, Wx, Wb and dgbias for the oracle's gyro_bias_correction and for the host's (hm::gyro_bias_correction behind the host
class's Core::gyroBiasCorrection, through tests/cpp/host_math_dump.cpp) - on what a chain of eleven pairs at ten different frame
intervals feeds it, and on the input families of the device glue's probe at the fourteen intervals of support.DT_GRID. The frame
interval and the two noise matrices, which the reference forms in rebvio.cpp around the call, are formed here in numpy.

The anchor. Core::tryVel (core.cpp:120-141) stores fabs(fi) as a keyline's residual although calculatefJ leaves fi unset on its
two early returns; fi is an uninitialised local. For a keyline that comes after a matched one the compiled code finds the matched
one's value there, which is the oracle's rule too ("Decisions for undefined behaviour"). BEFORE the first matched
keyline of a call the reference reads an indeterminate value (the oracle says 0): that residual, and through the next call's
weights the score and possibly the step of minimizeVel, is not a property of the reference but of one compilation. The cases here
do not exercise that read: where minimizeVel runs, or tryVel feeds residuals into a later call, keyline 0 of the searching map is
made an "anchor" - a copy of a keyline of the field's map in position, gradient and norm, at rho = RHO_MIN (a point so far away
that no velocity tried moves it by 0.1 px) - so that the first keyline evaluated always sets fi. That it did is asserted on the
reference's own output. test_try_vel also runs on the unchanged maps, from fresh residuals, and there the residuals below the
first forward-matched keyline are

NOT COMPARED, because the reference does not define them or gives no access:
  - tryVel's residuals of the keylines before the first forward-matched keyline of a call on un-anchored maps (above);
  - minimizeVel's score, velocity and covariance with a non-empty searching map against a field without a keyline (nothing can
    be anchored; the tiny-map cases pair a non-empty old map with a non-empty new one, and the empty new map with an empty old);
  - detection on a frame without a keyline: tuneThreshold reads keyline 0 of the empty map (edge_detector.cpp:168);
  - the scale images of ScaleSpace (private): scale0 / scale1 come from two FastGaussian objects built with the constructor
    arguments ScaleSpace gives its own; the detector's dense mask and auto threshold (private): the map's mask() and threshold()
    carry them; Core's DistanceField (private): a DistanceField of the driver's own, built from the same map;
  - minimizeVel's accept mask and quantile, extRotVel's JtF (not handed out); Core::testfk (inline, defined in core.cpp only:
    reached through calculatefJ); EdgeMapConfig off its defaults (EdgeDetector constructs every map with the defaults);
  - rebvio.cpp's statements around gyroBiasCorrection (frame_dt, RGyro, RGBias, Bg += dgbias, the SO3 correction) and the
    covariance P_V it takes from a Cholesky<6> inverse: rebvio.cpp is not compiled; the Cholesky of oracle/ref_shim, which the
    reference library and the three implementations compared with it share; Core::estimateBias and the two acceleration
    estimators (function-local statics; SABEstimator is not part of the library).
"""
import numpy as np
import pytest

from conftest import params_for
from support import host_lib, host_math_tool, ref_mod  # noqa: F401
from support import (DT_GRID, GLUE_GBC, KW_TRACK, RHO_MAX, RHO_MIN, STEPS_HEALTHY, TS, assert_keylines_equal, bits_equal, craft_writers, f32, frame_dt_of, glue_family,
                     glue_family_cases, gyro_noise, half_pixel_keylines, noise_frames, preset_targets, rodrigues, stamps_from, words)

H, W = 144, 192
TALLY = dict(keylines=0, pixels=0, scalars=0)
GBC = dict(calls=0, finite=0, words=0)
X_REL_MEASURED = 0.0   # largest |X_oracle - X_reference| / max|X_reference| seen by test_ext_rot_vel / the chain, printed by the tally


@pytest.fixture(scope="module", autouse=True)
def tally():
    yield
    print(f"\nreference pin: {TALLY['keylines']} keyline records, {TALLY['pixels']} pixels / field cells and {TALLY['scalars']} "
          f"scalars compared; largest relative deviation of extRotVel's X: {X_REL_MEASURED:.3g}; gyroBiasCorrection: {GBC['calls']} calls, "
          f"{GBC['finite']} with every output finite, {GBC['words']} words compared")


# ---- comparisons --------------------------------------------------------------------------------------------------------
def same_words(want, got, what):
    w, g = words(want), words(got)
    assert np.array_equal(w, g), f"{what}: reference {np.asarray(want).ravel()[:9]} oracle {np.asarray(got).ravel()[:9]}"
    TALLY["scalars"] += w.size


def same_image(want, got, what):
    assert want.shape == got.shape and bits_equal(want, got), f"{what}: {(want != got).sum()} of {want.size} pixels differ"
    TALLY["pixels"] += want.size


def same_map(mr, mo, what, mask=False):
    """size, every field of every keyline, the map threshold; with mask, the dense index mask too"""
    kr, ko = mr.keylines(), mo.keylines()
    assert_keylines_equal(kr, ko, what=what)
    same_words(mr.threshold, mo.threshold, f"{what}: map threshold")
    TALLY["keylines"] += len(kr)
    if mask:
        same_image(mr.mask(mr.ctx.rows, mr.ctx.cols), mo.mask(mr.ctx.rows, mr.ctx.cols), f"{what}: keyline mask")


# ---- the two libraries side by side ------------------------------------------------------------------------------------
class Sides:
    """a reference context and an oracle context with the same parameters, and the same detected maps in both"""

    def __init__(self, orc_mod, ref_mod, cam, **kw):
        self.p = params_for(orc_mod, cam, **kw)
        self.orc = orc_mod.Oracle(self.p)
        self.ref = ref_mod.Ref(self.p)
        self.rm, self.om = [], []

    def detect(self, frames):
        for i, f in enumerate(frames):
            self.rm.append(self.ref.detect_u8(f, i * TS))
            self.om.append(self.orc.detect_u8(f, i * TS))
        return self

    def load(self, k, kl, threshold=None):
        """the same keylines (and map threshold) into map k of both sides"""
        for m in (self.rm[k], self.om[k]):
            m.set_keylines(kl)
            if threshold is not None:
                m.threshold = threshold


def anchor(old_kl, new_kl, thr_old, thr_new):
    """(old_kl with keyline 0 made the anchor, the keyline of new_kl it copies) - or (old_kl, -1) when either map is empty. The
    copied keyline is the first one that stands at least a quarter pixel clear of a rounding boundary in both coordinates and passes
    both maps' gradient gates (core.hpp:47, core.cpp:88)."""
    if len(old_kl) == 0 or len(new_kl) == 0:
        return old_kl, -1
    frac = np.abs(new_kl["pos"] - np.round(new_kl["pos"])).max(1)
    ok = np.flatnonzero((frac < 0.25) & (new_kl["gradient_norm"] >= max(thr_old, thr_new, 0.0)))
    assert len(ok), "no keyline to anchor on"
    j = int(ok[0])
    out = old_kl.copy()
    for f in ("pos", "pos_img", "gradient", "gradient_norm"):
        out[f][0] = new_kl[f][j]
    out["rho"][0] = RHO_MIN
    out["sigma_rho"][0] = old_kl["sigma_rho"].min()
    return out, j


def glue(Vg, Xv, ok, R_prior):
    """What the pair body derives between extRotVel and directedMatch (rebvio.cpp:195-203, vision only), in numpy: it only has to
    hand both libraries the same numbers. A failed or non-finite solve counts as no correction."""
    Xv = np.asarray(Xv, np.float64)
    if not ok or not np.isfinite(Xv).all() or not np.isfinite(Vg).all():
        return np.zeros(3, np.float32), np.eye(3, dtype=np.float32), np.asarray(R_prior, np.float32)
    R0 = rodrigues(Xv[3:])
    V = R0 @ np.asarray(Vg, np.float64) + Xv[:3]
    return V.astype(np.float32), R0.astype(np.float32), (R0 @ np.asarray(R_prior, np.float64).T).T.astype(np.float32)


def pair_body(S, ko, kn, R_prior, fails=None, what="", lm=None):
    """One pair in the order of the reference's pair body (rebvio.cpp:142-259): buildDistanceField(new), rotateKeylines(old, prior),
    minimizeVel(old), forwardMatch(old -> new), extRotVel, rotateKeylines(old, correction), directedMatch(new <- old),
    regularize1Iter(new), updateInverseDepth. fails = None: the reference alone (warming). Otherwise the oracle runs every stage
    on the reference's outputs of the stage before - both of its maps are overwritten with the reference's after every stage - and
    each difference is appended to fails, so that one divergence does not hide the next. lm: a minimizeVel result to go on from
    (the maps then hold forward ids already): the prior rotation and minimizeVel are not run."""
    global X_REL_MEASURED
    ref, orc = S.ref, S.orc
    ro, rn, oo, on = S.rm[ko], S.rm[kn], S.om[ko], S.om[kn]
    both = fails is not None

    def check(stage, *scalars):
        if not both:
            return
        for name, r, o in scalars:
            try:
                same_words(r, o, f"{what} {stage}: {name}")
            except AssertionError as e:
                fails.append(str(e))
        for tag, mr, mo in (("old", ro, oo), ("new", rn, on)):
            try:
                same_map(mr, mo, f"{what} {stage}: {tag} map")
            except AssertionError as e:
                fails.append(str(e))
            mo.set_keylines(mr.keylines())
            mo.threshold = mr.threshold

    ref.build_distance_field(rn)
    if both:
        orc.build_distance_field(on)
        (ir, dr), (io, do) = ref.distance_field(), orc.distance_field()
        try:
            same_image(ir, io, f"{what} field ids")
            same_image(dr, do, f"{what} field distances")
        except AssertionError as e:
            fails.append(str(e))
    Rp = np.asarray(R_prior, np.float32)
    mr = lm
    if lm is None:
        ref.rotate(ro, Rp.T)
        if both:
            orc.rotate(oo, Rp.T)
        check("rotateKeylines(prior)")
        akl, j = anchor(ro.keylines(), rn.keylines(), ro.threshold, rn.threshold)
        S.load(ko, akl)
        mr = ref.minimize_vel(ro)
        if j >= 0:
            assert ro.keylines()["match_id_forward"][0] == j, f"{what}: the anchor did not match"
        if both:
            mo = orc.minimize_vel(oo)
            check("minimizeVel", ("vel", mr["vel"], mo["vel"]), ("Rvel", mr["Rvel"], mo["Rvel"]), ("score", mr["F"], mo["F"]))
    nr = ref.forward_match(ro, rn)
    if both:
        check("forwardMatch", ("count", nr, orc.forward_match(oo, on)))
    er = ref.ext_rot_vel(mr["vel"])
    if both:
        eo = orc.ext_rot_vel(mr["vel"])
        check("extRotVel", ("Wx", er["Wx"], eo["Wx"]), ("ok", er["ok"], eo["ok"]))
        if er["ok"] and np.isfinite(er["X"]).all() and np.abs(er["X"]).max() > 0:
            X_REL_MEASURED = max(X_REL_MEASURED, float(np.abs(eo["X"] - er["X"]).max() / np.abs(er["X"]).max()))
    V, R0, Rgva = glue(mr["vel"], er["X"], er["ok"], Rp)
    ref.rotate(ro, R0)
    if both:
        orc.rotate(oo, R0)
    check("rotateKeylines(correction)")
    Rvel = mr["Rvel"] if np.isfinite(mr["Rvel"]).all() else np.eye(3, dtype=np.float32)
    dr_ = ref.directed_match(rn, ro, V, Rvel, Rgva, S.p.search_range)
    if both:
        do_ = orc.directed_match(on, oo, V, Rvel, Rgva, S.p.search_range)
        check("directedMatch", ("count", dr_[0], do_[0]), ("keyframe matches", dr_[1], do_[1]))
    gr = ref.regularize(rn)
    if both:
        check("regularize1Iter", ("count", gr, orc.regularize(on)))
    ref.update_inverse_depth(V)
    if both:
        orc.update_inverse_depth(V)
    check("updateInverseDepth")
    return dict(klm=dr_[0], fwd=nr, reg=gr, V=V, Rvel=Rvel, Rgva=Rgva, vel=mr["vel"])


PRIOR = rodrigues([0.002, -0.003, 0.001]).astype(np.float32)   # a gyro prior of a few milliradians for every pair


@pytest.fixture(scope="module")
def warmed(orc_mod, ref_mod, small_stream):  # noqa: F811
    """Frames 0..5 detected on both sides, pairs 0-1, 1-2, 2-3 run on the reference alone, and the pair 3-4 up to forwardMatch: the
    keylines of maps 3 (old, rotated, anchored, forward ids set) and 4 (new, forward-matched) as arrays, the reference's
    minimizeVel result, and the anchor's target. Tests copy the arrays into maps of their own; nothing here is changed later."""
    frames, cam = small_stream
    S = Sides(orc_mod, ref_mod, cam, **KW_TRACK).detect(frames[:6])
    for k in range(3):
        out = pair_body(S, k, k + 1, PRIOR)
        assert out["klm"] > 300, out
    S.ref.build_distance_field(S.rm[4])
    S.ref.rotate(S.rm[3], PRIOR.T)
    before, j = anchor(S.rm[3].keylines(), S.rm[4].keylines(), S.rm[3].threshold, S.rm[4].threshold)
    S.rm[3].set_keylines(before)
    new_before = S.rm[4].keylines()
    mr = S.ref.minimize_vel(S.rm[3])
    old_lm = S.rm[3].keylines()
    S.ref.forward_match(S.rm[3], S.rm[4])
    return dict(cam=cam, frames=frames, old_before=before, new_before=new_before, old_lm=old_lm, new_fwd=S.rm[4].keylines(), lm=mr,
                anchor=j, thr_old=S.rm[3].threshold, thr_new=S.rm[4].threshold)


def fresh_sides(orc_mod, ref_mod, warmed, **kw):
    """contexts of their own with frames 0..4 detected (the maps' masks and thresholds), maps 3 and 4 to be loaded by the test"""
    return Sides(orc_mod, ref_mod, warmed["cam"], **dict(KW_TRACK, **kw)).detect(warmed["frames"][:5])


# ---- scale space and smooth --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image", ["stream", "constant"])
def test_scale_space_and_smooth(orc_mod, ref_mod, small_stream, image):  # noqa: F811
    """scale0, scale1, dog, mag (borders included) and the six filter widths; FastGaussian.smooth at three (sigma, n)."""
    frames, cam = small_stream
    S = Sides(orc_mod, ref_mod, cam, **KW_TRACK)
    img = frames[5].astype(np.float32) * np.float32(3.0) if image == "stream" else np.full((H, W), 381.0, np.float32)
    sr, so = S.ref.scale_space(img), S.orc.scale_space(img)
    for k in ("scale0", "scale1", "dog", "mag"):
        same_image(sr[k], so[k], f"{image}: {k}")
    for f in range(2):
        for k in range(3):
            assert S.ref.filter_width(f, k) == S.orc.L.orc_filter_width(S.orc.h, f, k)
    for sigma, n in ((3.56359, 3), (2.2, 4), (4.49, 2)):
        (a, wa), (b, wb) = S.ref.smooth(img, sigma, n), S.orc.smooth(img, sigma, n)
        assert wa == wb, (sigma, n, wa, wb)
        same_image(a, b, f"{image}: smooth({sigma}, {n})")


# ---- detection ------------------------------------------------------------------------------------------------------------
DETECT = {
    "default": KW_TRACK,
    "combined-gates": dict(keylines_ref=1500, keylines_max=6000, gain=0.0, pos_neg_threshold=0.2, dog_threshold=0.3, threshold=0.005),
    "servo-swing": dict(keylines_max=6000, gain=5e-5, keylines_ref=1500),   # BASE + COMBINED and SERVO["swing"] of test_detect_params_gpu
}


@pytest.mark.parametrize("name", list(DETECT))
def test_detect_twelve_frames(orc_mod, ref_mod, small_stream, name):  # noqa: F811
    """Twelve consecutive frames: after each, every keyline field, the map's mask, its threshold (the auto threshold), the count
    and the detector's servo threshold. The servo has to move where it is on."""
    frames, cam = small_stream
    S = Sides(orc_mod, ref_mod, cam, **DETECT[name])
    servo = []
    for i in range(12):
        mr, mo = S.ref.detect_u8(frames[i], i * TS), S.orc.detect_u8(frames[i], i * TS)
        assert mr.size() > 100, (name, i, mr.size())
        same_map(mr, mo, f"{name} frame {i}", mask=True)
        same_words(S.ref.threshold, S.orc.threshold, f"{name} frame {i}: servo threshold")
        servo.append(S.ref.threshold)
    assert (len(set(servo)) > 6) == (DETECT[name].get("gain", 5e-7) > 0), (name, servo)


@pytest.mark.parametrize("size", [(32, 32), (33, 35)], ids=["32x32", "33x35"])
def test_detect_small_sizes(orc_mod, ref_mod, size):  # noqa: F811
    from rebvio_amd import synth
    w, h = size
    frames = noise_frames(w, h, 4, seed=w * h)
    cam = synth.Camera(w, h, 100.0, 0.5 * w, 0.5 * h)
    S = Sides(orc_mod, ref_mod, cam, keylines_ref=150, keylines_max=400)
    img = frames[0].astype(np.float32) * np.float32(3.0)
    sr, so = S.ref.scale_space(img), S.orc.scale_space(img)
    for k in ("scale0", "scale1", "dog", "mag"):
        same_image(sr[k], so[k], f"{w}x{h}: {k}")
    for i in range(4):
        mr, mo = S.ref.detect_u8(frames[i], i * TS), S.orc.detect_u8(frames[i], i * TS)
        assert mr.size() > 10, (size, i, mr.size())
        same_map(mr, mo, f"{w}x{h} frame {i}", mask=True)
        same_words(S.ref.threshold, S.orc.threshold, f"{w}x{h} frame {i}: servo threshold")


# ---- distance field ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["default", "range-10", "map-threshold", "half-pixel-ties"])
def test_distance_field(orc_mod, ref_mod, warmed, case):  # noqa: F811
    """id and distance at every cell: search range 40 and 10, with a positive map threshold (the median gradient norm, so that half
    of the keylines are gated out), and with keylines whose cells are all rounding ties, at the borders; built twice, so that cells
    a rebuild leaves keep their stale distance on both sides."""
    S = fresh_sides(orc_mod, ref_mod, warmed, **(dict(search_range=10.0) if case == "range-10" else {}))
    kl = half_pixel_keylines(warmed["new_fwd"], W, H) if case == "half-pixel-ties" else warmed["new_fwd"]
    S.load(4, kl, f32(np.median(kl["gradient_norm"])) if case == "map-threshold" else f32(0.0 if case == "half-pixel-ties" else warmed["thr_new"]))
    for k in (3, 4):
        S.ref.build_distance_field(S.rm[k])
        S.orc.build_distance_field(S.om[k])
        (ir, dr), (io, do) = S.ref.distance_field(), S.orc.distance_field()
        assert (ir >= 0).sum() > 2000
        same_image(ir, io, f"{case}: ids of map {k}")
        same_image(dr, do, f"{case}: distances of map {k}")
    if case == "half-pixel-ties":   # the ties decide cells: keylines 0..47 own some, and column 0 / row 0 next to a -0.5 tie are not theirs
        assert np.isin(np.arange(48), ir).sum() >= 40


# ---- rotateKeylines, estimateQuantile ------------------------------------------------------------------------------------
def test_rotate_and_quantile(orc_mod, ref_mod, warmed):  # noqa: F811
    """the rotation and the percentile / bin pairs of test_parity_gpu.test_rotate_and_quantile_bit_exact, on a map with depths"""
    S = fresh_sides(orc_mod, ref_mod, warmed)
    S.load(4, warmed["new_fwd"])
    a = 0.004
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    R = (R @ np.array([[1, 0, 0], [0, np.cos(0.002), -np.sin(0.002)], [0, np.sin(0.002), np.cos(0.002)]], np.float32)).astype(np.float32)
    for k in (3, 4):
        for pct, bins in ((0.9, 100), (0.5, 37), (0.99, 128)):
            same_words(S.ref.quantile(S.rm[k], pct, bins), S.orc.quantile(S.om[k], pct, bins), f"quantile({pct}, {bins}) of map {k}")
        S.ref.rotate(S.rm[k], R)
        S.orc.rotate(S.om[k], R)
        same_map(S.rm[k], S.om[k], f"rotateKeylines of map {k}")


# ---- tryVel ------------------------------------------------------------------------------------------------------------------
VELS = ([0, 0, 0], [-0.011, -0.005, -0.003], [0.02, 0.01, -0.9])   # test_parity_gpu.test_try_vel_parity


@pytest.mark.parametrize("anchored", [True, False], ids=["anchored", "unchanged-maps"])
def test_try_vel(orc_mod, ref_mod, warmed, anchored):  # noqa: F811
    """Score, JtJ, JtF, the residual array and every keyline (the forward ids) at zero and two non-zero velocities.
    anchored: the residuals of one call weigh the next, and all of them are compared. unchanged-maps: the warmed map without the
    anchor, every call from residuals of zero; residuals are compared from the first forward-matched keyline on (module docstring)."""
    S = fresh_sides(orc_mod, ref_mod, warmed)
    old = warmed["old_before"].copy()
    if not anchored:
        old[0] = S.rm[3].keylines()[0]   # the detected keyline 0, fresh depth: no anchor
    S.load(3, old, warmed["thr_old"])
    S.load(4, warmed["new_before"], warmed["thr_new"])
    S.ref.build_distance_field(S.rm[4])
    S.orc.build_distance_field(S.om[4])
    srm = S.ref.quantile(S.rm[3])
    n = len(old)
    res_r, res_o = np.zeros(n, np.float32), np.zeros(n, np.float32)
    matched = []
    for vel in VELS:
        if not anchored:
            res_r[:], res_o[:] = 0, 0
        sr, Jr, Fr = S.ref.try_vel(S.rm[3], vel, srm, res_r)
        so, Jo, Fo = S.orc.try_vel(S.om[3], vel, srm, res_o)
        same_words(sr, so, f"tryVel {vel}: score")
        same_words(Jr, Jo, f"tryVel {vel}: JtJ")
        same_words(Fr, Fo, f"tryVel {vel}: JtF")
        same_map(S.rm[3], S.om[3], f"tryVel {vel}")
        fwd = S.rm[3].keylines()["match_id_forward"]
        matched.append(int((fwd >= 0).sum()))
        first = 0
        if anchored:
            assert fwd[0] == warmed["anchor"], (vel, fwd[0])
        else:
            first = int(np.argmax(fwd >= 0)) if matched[-1] else n
        same_words(res_r[first:], res_o[first:], f"tryVel {vel}: residuals from keyline {first}")
    assert matched[0] > 500 and matched[1] > 500, matched


# ---- minimizeVel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [(0.0, 0.0, 0.0), (0.05, 0.0, 0.0)], ids=["from-zero", "from-0.05"])
def test_minimize_vel(orc_mod, ref_mod, warmed, start):  # noqa: F811
    """vel, Rvel, the score and every keyline (match_id_forward) after the five Levenberg-Marquardt iterations."""
    S = fresh_sides(orc_mod, ref_mod, warmed)
    S.load(3, warmed["old_before"], warmed["thr_old"])
    S.load(4, warmed["new_before"], warmed["thr_new"])
    S.ref.build_distance_field(S.rm[4])
    S.orc.build_distance_field(S.om[4])
    r, o = S.ref.minimize_vel(S.rm[3], start), S.orc.minimize_vel(S.om[3], start)
    fwd = S.rm[3].keylines()["match_id_forward"]
    assert fwd[0] == warmed["anchor"] and (fwd >= 0).sum() > 500
    assert np.abs(r["vel"] - np.array(start, np.float32)).max() > 1e-4   # (the run moved)
    for k in ("vel", "Rvel", "F"):
        same_words(r[k], o[k], f"minimizeVel from {start}: {k}")
    same_map(S.rm[3], S.om[3], f"minimizeVel from {start}")


# ---- forwardMatch, directedMatch, regularize1Iter, updateInverseDepth on crafted maps --------------------------------
@pytest.mark.parametrize("layout,pattern", [("contiguous", "shared_max"), ("stride6", "clamps")])
def test_forward_match_crafted(orc_mod, ref_mod, warmed, layout, pattern):  # noqa: F811
    """two of support's crafted forwardMatch maps (groups of 1 .. 600 writers per target, shared maxima / both clamps), the targets
    pre-matched at every relation of rho the gate at edge_map.cpp:83 tells apart; then the rest of the pair body on what it left"""
    S = fresh_sides(orc_mod, ref_mod, warmed)
    base = warmed["old_lm"].copy()
    base["rho"] = np.clip(base["rho"], RHO_MIN, RHO_MAX)   # (the prior rotation took a clamped depth a rounding past its clamp)
    old, groups = craft_writers(base, len(warmed["new_before"]), layout, pattern)
    new, _ = preset_targets(warmed["new_before"], old, groups)
    S.load(3, old, warmed["thr_old"])
    S.load(4, new, warmed["thr_new"])
    fails = []
    out = pair_body(S, 3, 4, PRIOR, fails, what=f"crafted {layout} {pattern}", lm=warmed["lm"])
    assert not fails, "\n".join(fails[:12])
    assert out["fwd"] > 100 and out["klm"] > 100, out


def test_match_regularize_depth_stages(orc_mod, ref_mod, warmed):  # noqa: F811
    """directedMatch, regularize1Iter, updateInverseDepth one after the other on the warmed pair: the counters and every field of
    every keyline of both maps after each call (inputs of each call: the reference's outputs of the one before, equal when green)."""
    S = fresh_sides(orc_mod, ref_mod, warmed)
    S.load(3, warmed["old_lm"], warmed["thr_old"])
    S.load(4, warmed["new_fwd"], warmed["thr_new"])
    S.ref.build_distance_field(S.rm[4])
    S.orc.build_distance_field(S.om[4])
    V, Rvel = warmed["lm"]["vel"], warmed["lm"]["Rvel"]
    a = 0.0007
    Rb = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    dr, do = S.ref.directed_match(S.rm[4], S.rm[3], V, Rvel, Rb), S.orc.directed_match(S.om[4], S.om[3], V, Rvel, Rb)
    assert dr[0] > 300
    same_words(dr, do, "directedMatch counters")
    same_map(S.rm[4], S.om[4], "directedMatch: new map")
    same_map(S.rm[3], S.om[3], "directedMatch: old map")
    gr, go = S.ref.regularize(S.rm[4]), S.orc.regularize(S.om[4])
    assert gr > 100
    same_words(gr, go, "regularize1Iter count")
    same_map(S.rm[4], S.om[4], "regularize1Iter")
    S.ref.update_inverse_depth(V)
    S.orc.update_inverse_depth(V)
    same_map(S.rm[4], S.om[4], "updateInverseDepth")
    assert (S.rm[4].keylines()["rho"] != warmed["new_fwd"]["rho"]).sum() > 300


# ---- searchMatch, keyline by keyline ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["velocity", "degenerate"])
def test_search_match_every_keyline(orc_mod, ref_mod, warmed, case):  # noqa: F811
    """the returned index for every keyline of the new map searched in the old one; degenerate: zero velocity, |t| <= 1e-6, the
    search runs along the keyline's own gradient (edge_map.cpp:138-148)"""
    S = fresh_sides(orc_mod, ref_mod, warmed)
    S.load(3, warmed["old_lm"])
    queries = warmed["new_fwd"]
    eye = np.eye(3, dtype=np.float32)
    if case == "velocity":
        V, Rvel, Rb = warmed["lm"]["vel"], warmed["lm"]["Rvel"], rodrigues([0, 0.0007, 0]).astype(np.float32)
    else:
        V, Rvel, Rb = np.zeros(3, np.float32), eye * np.float32(1e-6), eye
    want = np.array([S.ref.search_match(S.rm[3], q, V, Rvel, Rb) for q in queries])
    got = np.array([S.orc.search_match(S.om[3], q, V, Rvel, Rb) for q in queries])
    assert (want >= 0).sum() > 50, (case, (want >= 0).sum())
    assert np.array_equal(want, got), (case, np.flatnonzero(want != got)[:8])
    TALLY["keylines"] += len(queries)


# ---- calculatefJ and updateInverseDepthARLU, one keyline at a time ------------------------------------------------------
def test_single_keyline_forms(orc_mod, ref_mod, warmed):  # noqa: F811
    """Core::calculatefJ for every old keyline at the cell it stands on (matched, gradient-rejected and empty cells all occur; an
    output the call leaves unset reads the 0 it held before) and Core::updateInverseDepthARLU on every forward-matched new keyline."""
    import ctypes as C
    S = fresh_sides(orc_mod, ref_mod, warmed)
    S.load(4, warmed["new_fwd"], warmed["thr_new"])
    S.ref.build_distance_field(S.rm[4])
    S.orc.build_distance_field(S.om[4])
    kinds = set()
    for k in warmed["old_lm"][::4]:
        x, y = int(k["pos"][0] + 0.5), int(k["pos"][1] + 0.5)
        fr, dxr, dyr, mr, fir, kr = S.ref.calculate_fj(y * W + x, k, float(k["pos"][0]), float(k["pos"][1]))
        q = np.array([k])
        dx, dy, fi, mn = C.c_float(0), C.c_float(0), C.c_float(0), C.c_int(0)
        fo = S.orc.L.orc_calculate_fj(S.orc.h, y * W + x, C.byref(dx), C.byref(dy), q.ctypes.data, float(k["pos"][0]), float(k["pos"][1]),
                                      C.byref(mn), C.byref(fi))
        same_words([fr, dxr, dyr, fir], [fo, dx.value, dy.value, fi.value], "calculatefJ outputs")
        assert mr == mn.value and kr["match_id_forward"] == q[0]["match_id_forward"]
        kinds.add(mr)
    assert kinds == {0, 1}
    V = warmed["lm"]["vel"]
    vv, pv = np.ascontiguousarray(V, np.float32), None
    pv = vv.ctypes.data_as(C.POINTER(C.c_float))
    done = 0
    for k in warmed["new_fwd"][warmed["new_fwd"]["match_id"] >= 0][::2]:
        kr = S.ref.update_inverse_depth_arlu(k, V)
        q = np.array([k])
        S.orc.L.orc_update_inverse_depth_arlu(S.orc.h, q.ctypes.data, pv)
        assert_keylines_equal(np.array([kr]), q, what="updateInverseDepthARLU")
        done += 1
    assert done > 150
    TALLY["keylines"] += done


# ---- extRotVel ------------------------------------------------------------------------------------------------------------------
X_REL_MEASURED_HERE = 0.0           # the largest relative deviation of X measured on the inputs of this file (docstring below)
X_REL_BAR = 4 * X_REL_MEASURED_HERE


def test_ext_rot_vel(orc_mod, ref_mod, warmed):  # noqa: F811
    """Wx and the return flag bit for bit, at the LM velocity and at zero. EQUAL X SAYS NOTHING ABOUT THE REFERENCE'S SOLVER: TooN's
    SVD<6>::backsub calls LAPACK's gesvd, which is not available, so both sides solve with a cyclic-Jacobi stand-in (oracle:
    sym_pinv_solve in rebvio_oracle.cpp; reference library: oracle/ref_shim/TooN/SVD.h). The two routines are written separately and
    are not one shared routine, so the bar for X is four times the largest relative deviation max|X_oracle - X_reference| /
    max|X_reference| measured against the reference library on these inputs (the convention of test_hotpath_math.py). Measured: 0 in
    both cases of this test and in every extRotVel call of the chain tests (both routines work in double and round to the same
    floats), so the bar is 0 - X has to be equal as floats - which is below the 5e-3 the project uses for X elsewhere. The tally
    printed at the end of the module reports the value again. What this test pins is the matrix and, through X, the right-hand side
    the solve starts from - not the solve."""
    global X_REL_MEASURED
    S = fresh_sides(orc_mod, ref_mod, warmed)
    S.load(4, warmed["new_fwd"], warmed["thr_new"])
    S.ref.build_distance_field(S.rm[4])
    S.orc.build_distance_field(S.om[4])
    assert (warmed["new_fwd"]["match_id"] >= 0).sum() > 300
    for vel in (warmed["lm"]["vel"], np.zeros(3, np.float32)):
        r, o = S.ref.ext_rot_vel(vel), S.orc.ext_rot_vel(vel)
        assert r["ok"] == 1
        same_words(r["ok"], o["ok"], "extRotVel flag")
        same_words(r["Wx"], o["Wx"], "extRotVel Wx")
        rel = float(np.abs(o["X"] - r["X"]).max() / np.abs(r["X"]).max())
        X_REL_MEASURED = max(X_REL_MEASURED, rel)
        print(f"extRotVel X: relative deviation {rel:.3g} (bar {X_REL_BAR:.3g})")
        assert X_REL_BAR <= 5e-3 and rel <= X_REL_BAR, (rel, r["X"], o["X"])


# ---- the chain ------------------------------------------------------------------------------------------------------------------
def test_chain_of_four_pairs(orc_mod, ref_mod, small_stream):  # noqa: F811
    """Frames 0..4, four consecutive pairs with the stages in the order of the reference's pair body, so that depths, match counts
    and forward ids are warmed state; both libraries driven by pair_body, compared after every stage of every pair."""
    frames, cam = small_stream
    S = Sides(orc_mod, ref_mod, cam, **KW_TRACK).detect(frames[:5])
    fails = []
    for k in range(4):
        out = pair_body(S, k, k + 1, PRIOR, fails, what=f"pair {k}-{k + 1}")
        assert out["klm"] > 300 and out["fwd"] > 300 and (k == 0 or out["reg"] > 100), (k, out)
    assert not fails, "\n".join(fails[:12])
    assert (S.rm[4].keylines()["matches"] >= 3).sum() > 100   # (state that only a chain builds)


@pytest.mark.parametrize("n_old,n_new", [(0, None), (1, None), (2, None), (None, 1), (None, 2), (0, 0)],
                         ids=["old-0", "old-1", "old-2", "new-1", "new-2", "both-0"])
def test_chain_tiny_maps(orc_mod, ref_mod, warmed, n_old, n_new):  # noqa: F811
    """The pair body with a map cut to its first 0, 1 or 2 keylines (None: the whole warmed map), as in the tiny-map tests of
    test_keyline_counts_gpu. A non-empty old map against an EMPTY new one is left out: nothing can be anchored (module docstring)."""
    S = fresh_sides(orc_mod, ref_mod, warmed)
    old, new = warmed["old_before"], warmed["new_before"].copy()
    new["id_prev"][:2], new["id_next"][:2] = -1, -1   # (the cut map keeps no link out of itself)
    S.load(3, old if n_old is None else old[:n_old], warmed["thr_old"])
    S.load(4, new if n_new is None else new[:n_new], warmed["thr_new"])
    fails = []
    pair_body(S, 3, 4, np.eye(3, dtype=np.float32), fails, what=f"tiny {n_old}/{n_new}")
    assert not fails, "\n".join(fails[:12])


# ---- gyroBiasCorrection ---------------------------------------------------------------------------------------------------------
GBC_OUTPUTS = ("X", "Wx", "Wb", "dgbias")


def noise_matrices(p, dt):
    """RGyro, RGBias of a pair at the interval dt (rebvio.cpp:186-187), in numpy"""
    s_g, s_b = gyro_noise(p, dt)
    return np.eye(3, dtype=np.float32) * s_g, np.eye(3, dtype=np.float32) * s_b


def same_gbc(want, got, what):
    """X, Wx, Wb and dgbias of two gyroBiasCorrection results, word for word; every difference named at once"""
    bad = [f"{name}: reference {np.ravel(r)[:6]} got {np.ravel(g)[:6]}" for name, r, g in zip(GBC_OUTPUTS, want, got)
           if not np.array_equal(words(r), words(g))]
    assert not bad, f"{what}: " + "; ".join(bad)
    GBC["words"] += sum(np.size(r) for r in want)


def host_gbc(tool, X, Wx, Wb, Rg, Rb):
    """the host class's Core::gyroBiasCorrection (which is hm::gyro_bias_correction, rebvio_amd/host/core.cpp) through the gbc mode
    of tests/cpp/host_math_dump.cpp, in the shapes of the two bindings"""
    out = tool("gbc", np.concatenate([np.ravel(a).astype(np.float32) for a in (X, Wx, Wb, Rg, Rb)]))
    return out[:6], out[6:42].reshape(6, 6), out[42:51].reshape(3, 3), out[51:54]


def test_gyro_bias_correction_on_a_real_chain(orc_mod, ref_mod, small_stream, host_math_tool):  # noqa: F811
    """Core::gyroBiasCorrection of the reference library against the oracle's and the host's on what a chain of pairs feeds it: Xv and
    W_Xv of the eleven pairs of small_stream at the intervals of STEPS_HEALTHY (the oracle's track_pair, default sum order), the noise
    matrices of each pair's interval, W_Bg carried from pair to pair as the REFERENCE leaves it. The oracle's own pair step must have
    been handed the same: its Xgv and its state after the pair are the reference's X and Wb, its Bg the running sum of dgbias."""
    frames, cam = small_stream
    p = params_for(orc_mod, cam, **KW_TRACK)
    orc, ref = orc_mod.Oracle(p), ref_mod.Ref(p)
    ts = stamps_from(STEPS_HEALTHY)
    Bg, W_Bg = orc.gyro_state()
    prev = None
    for k in range(len(ts)):
        m = orc.detect_u8(frames[k], ts[k])
        if prev is not None:
            dt = frame_dt_of(ts[k - 1], ts[k])
            po = orc.track_pair(prev, m, frame_dt=dt)
            assert po.status == 0 and po.klm_num > 1000, (k, po.status, po.klm_num)
            Rg, Rb = noise_matrices(p, dt)
            args = (np.array(po.Xv, np.float32), np.array(po.W_Xv, np.float32), W_Bg, Rg, Rb)
            want = ref.gyro_bias_correction(*args)
            assert all(np.isfinite(a).all() for a in want), (k, dt)
            same_gbc(want, orc_mod.gyro_bias_correction(*args), f"pair {k} (dt {dt}): oracle")
            same_gbc(want, host_gbc(host_math_tool, *args), f"pair {k} (dt {dt}): host")
            Bg = (Bg + want[3]).astype(np.float32)
            W_Bg = want[2]
            same_words(want[0], po.Xgv, f"pair {k}: Xgv of the oracle's pair record")
            same_words(W_Bg, orc.gyro_state()[1], f"pair {k}: W_Bg of the oracle's state")
            same_words(Bg, orc.gyro_state()[0], f"pair {k}: Bg of the oracle's state")
            GBC["calls"] += 1
            GBC["finite"] += 1
        prev = m
    assert len(set(frame_dt_of(a, b) for a, b in zip(ts, ts[1:]))) == 10   # (ten different intervals in eleven pairs)


_gbc_grid = {}


def gbc_grid(orc_mod, ref_mod):
    """the reference's result for every family, decade of W_Bg and dt of the grid - computed once - and the precondition on it:
    some dt leaves every output of every family but the NaN one finite, and at least three leave a non-finite Wb"""
    if not _gbc_grid:
        p = orc_mod.default_params(H, W)
        ref = ref_mod.Ref(p)
        for fam, decade in glue_family_cases():
            g = glue_family(fam, decade)
            for dt in DT_GRID:
                args = (g["X"], g["Wx"], g["W_Bg"]) + noise_matrices(p, dt)
                _gbc_grid[fam, decade, dt] = (args, ref.gyro_bias_correction(*args))
        finite = {k: all(np.isfinite(a).all() for a in want) for k, (_, want) in _gbc_grid.items()}
        clean = [dt for dt in DT_GRID if all(v for (fam, _, d), v in finite.items() if d == dt and fam != "nan-entry")]
        broken = [dt for dt in DT_GRID if any(not np.isfinite(want[2]).all() for (_, _, d), (_, want) in _gbc_grid.items() if d == dt)]
        assert len(clean) >= 1 and len(broken) >= 3, (clean, broken)
        assert all(not v for (fam, _, _), v in finite.items() if fam == "nan-entry")
        GBC["calls"] += len(finite)
        GBC["finite"] += sum(finite.values())
    return _gbc_grid


@pytest.mark.parametrize("side", ["oracle", "host"])
def test_gyro_bias_correction_on_the_probe_families(orc_mod, ref_mod, host_math_tool, side):  # noqa: F811
    """The input families of the device glue's probe (support.glue_family: a well-conditioned system, a rank-deficient one, a zero
    rotational block, a NaN entry, W_Bg at nine decades) at every interval of DT_GRID, which runs from 1 s through the intervals
    whose s_g^3 is a denormal or zero in fp32 to a repeated stamp and a stamp that goes back: the oracle's function, and the
    host's (the one hm::gyro_bias_correction behind Core::gyroBiasCorrection and the per-pair API), against the reference's."""
    for (fam, decade, dt), (args, want) in gbc_grid(orc_mod, ref_mod).items():
        got = orc_mod.gyro_bias_correction(*args) if side == "oracle" else host_gbc(host_math_tool, *args)
        same_gbc(want, got, f"{side}: {fam}, W_Bg ~ 1e{decade}, dt {dt}")


def test_recorded_gyro_bias_correction_results_are_the_reference(orc_mod, ref_mod):  # noqa: F811
    """tests/golden/glue_gbc_reference.npz, which tests/test_reference_pin_gpu.py holds the device glue to where the library cannot
    be rebuilt: X, Wx, Wb and dgbias recorded there are what the live library returns for the recorded Xv and W_Xv (the device
    glue's own, which that test checks), and what the oracle's function returns."""
    rec = np.load(GLUE_GBC)
    p = orc_mod.default_params(96, 128)
    ref = ref_mod.Ref(p)
    cases = [(fam, decade, dt) for fam, decade in glue_family_cases() for dt in DT_GRID]
    assert len(rec["X"]) == len(cases)
    for k, (fam, decade, dt) in enumerate(cases):
        args = (rec["Xv"][k], rec["W_Xv"][k], glue_family(fam, decade)["W_Bg"]) + noise_matrices(p, dt)
        want = ref.gyro_bias_correction(*args)
        recorded = (rec["X"][k], rec["Wx"][k].reshape(6, 6), rec["Wb"][k].reshape(3, 3), rec["dgbias"][k])
        same_gbc(want, recorded, f"recorded: {fam}, W_Bg ~ 1e{decade}, dt {dt}")
        same_gbc(want, orc_mod.gyro_bias_correction(*args), f"oracle on the device's inputs: {fam}, W_Bg ~ 1e{decade}, dt {dt}")
        GBC["calls"] += 1
        GBC["finite"] += int(all(np.isfinite(a).all() for a in want))
