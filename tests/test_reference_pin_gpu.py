"""The HIP entry points against the reference's own compiled hot path (oracle/_ref/librebvio_ref.so, see test_reference_pin.py),
without the oracle in between: detect, the distance field, directed_match, regularize and update_inverse_depth - the stages with no
sum-order freedom - over three chained 192x144 pairs, every keyline field bit for bit. The library travels with the tree; nothing is
read from the reference checkout here (the ref_mod fixture builds only where a checkout is present, and skips only when there is
neither a checkout nor a library).

The stages between the field and directed_match (rotateKeylines, minimizeVel, forwardMatch, extRotVel) run on the reference alone
and their result is uploaded into the device's maps: their sums are order-dependent on the device and test_parity_gpu holds them to
the oracle, which test_reference_pin.py holds to this library.

The device form of the pair glue (rebvio_hip_test_glue: glue_dev.hpp's workgroup, the gyroBiasCorrection matrices formed on the
device) is held to the library's Core::gyroBiasCorrection, on the probe's input families at every interval of DT_GRID, through
results of the library recorded under tests/golden/ (the test says why).
"""
import numpy as np
import pytest

from conftest import params_for
from support import B, ref_mod  # noqa: F401
from support import DT_GRID, GLUE_GBC, KW_TRACK, TS, assert_keylines_equal, bits_equal, glue_family, glue_family_cases, half_pixel_keylines, rodrigues, words

pytestmark = pytest.mark.gpu

PRIOR = rodrigues([0.002, -0.003, 0.001]).astype(np.float32)


def assert_map_equal(mr, gm, what, mask=False):
    assert_keylines_equal(mr.keylines(), gm.keylines(), what=what)
    assert bits_equal(np.float32(mr.threshold), np.float32(gm.threshold)), (what, mr.threshold, gm.threshold)
    if mask:
        assert np.array_equal(mr.mask(mr.ctx.rows, mr.ctx.cols), gm.mask()), f"{what}: keyline mask"


def test_hip_stages_against_the_reference_library(ref_mod, B, small_stream):  # noqa: F811
    frames, cam = small_stream
    ref = ref_mod.Ref(params_for(ref_mod, cam, **KW_TRACK))
    ctx = B.Context(params_for(B, cam, **KW_TRACK))
    rm = [ref.detect_u8(frames[0], 0)]
    gm = [ctx.detect_u8(frames[0], 0)]
    assert_map_equal(rm[0], gm[0], "detect frame 0", mask=True)
    for k in range(1, 4):
        rm.append(ref.detect_u8(frames[k], k * TS))
        gm.append(ctx.detect_u8(frames[k], k * TS))
        ro, rn, go, gn = rm[-2], rm[-1], gm[-2], gm[-1]
        assert rn.size() > 1000
        assert_map_equal(rn, gn, f"detect frame {k}", mask=True)
        assert_map_equal(ro, go, f"pair {k}: the old map as the pair before left it")   # (the chain: the device's own state)
        # the distance field of the new map
        ref.build_distance_field(rn)
        ctx.build_distance_field(gn)
        (ir, dr), (ig, dg) = ref.distance_field(), ctx.distance_field()
        assert np.array_equal(ir, ig), f"pair {k}: field ids differ in {(ir != ig).sum()} cells"
        assert (ir >= 0).sum() > 2000 and np.array_equal(dr[ir >= 0], dg[ir >= 0]), f"pair {k}: field distances"
        # the order-dependent stages, on the reference alone (rebvio.cpp:166-203, vision only); the device's maps take the result
        ref.rotate(ro, PRIOR.T)
        lm = ref.minimize_vel(ro)
        assert ref.forward_match(ro, rn) > 300
        ext = ref.ext_rot_vel(lm["vel"])
        assert ext["ok"] == 1 and np.isfinite(ext["X"]).all()
        R0 = rodrigues(ext["X"][3:].astype(np.float64))
        V = (R0 @ lm["vel"].astype(np.float64) + ext["X"][:3]).astype(np.float32)
        Rgva = (R0 @ PRIOR.astype(np.float64).T).T.astype(np.float32)
        ref.rotate(ro, R0.astype(np.float32))
        go.upload(ro.keylines())
        gn.upload(rn.keylines())
        # directedMatch, regularize1Iter, updateInverseDepth
        nr, kr = ref.directed_match(rn, ro, V, lm["Rvel"], Rgva, 40.0)
        ng, kg = ctx.directed_match(gn, go, V, lm["Rvel"], Rgva, 40.0)
        assert (nr, kr) == (ng, kg) and nr > 300, (k, nr, kr, ng, kg)
        assert_map_equal(rn, gn, f"pair {k}: directedMatch")
        cr, cg = ref.regularize(rn), ctx.regularize(gn)
        assert cr == cg and (k == 1 or cr > 100), (k, cr, cg)
        assert_map_equal(rn, gn, f"pair {k}: regularize1Iter")
        ref.update_inverse_depth(V)
        ctx.update_inverse_depth(V)
        assert_map_equal(rn, gn, f"pair {k}: updateInverseDepth")
        gm.pop(0).release()
        rm.pop(0)
    assert (rm[-1].keylines()["matches"] >= 2).sum() > 100   # (depth state a chain builds)
    # the distance field where every cell coordinate is a rounding tie, at the borders (support.half_pixel_keylines)
    ties = half_pixel_keylines(rm[-1].keylines(), cam.width, cam.height)
    rm[-1].set_keylines(ties)
    gm[-1].upload(ties)
    ref.build_distance_field(rm[-1])
    ctx.build_distance_field(gm[-1])
    (ir, dr), (ig, dg) = ref.distance_field(), ctx.distance_field()
    assert np.array_equal(ir, ig), f"ties: field ids differ in {(ir != ig).sum()} cells, first {np.argwhere(ir != ig)[:4].tolist()}"
    assert np.array_equal(dr[ir >= 0], dg[ir >= 0]), "ties: field distances"
    ctx.close()


def test_device_glue_against_the_reference_gyro_bias_correction(B):  # noqa: F811
    """rebvio_hip_test_glue on support.glue_family at every dt of DT_GRID against what the reference's Core::gyroBiasCorrection
    returned for the glue's own Xv and W_Xv, the W_Bg handed in and diag(s_g), diag(s_b) of the interval. The reference library can
    be built only where the reference checkout is, and a library that travelled with the tree may predate the driver's entry, so
    its results are recorded: tests/golden/glue_gbc_reference.npz (tests/golden/make_glue_gbc.py), which
    tests/test_reference_pin.py holds to the live library. Here: the device record's Xv and W_Xv are the recorded inputs (else the
    record is of something else and the test fails there), its Xgv is the reference's X, the state's W_Bg its Wb, the state's Bg
    the Bg handed in plus its dgbias (one fp32 add per element) - word for word, a NaN a NaN. The host form of the same call
    (glue.hpp, what the per-pair API runs) is held to the same values. Asserted on the recorded output before the device is
    looked at: some dt leaves every output of every family but the NaN one finite, at least three leave a non-finite Wb."""
    rec = np.load(GLUE_GBC)
    cases = [(fam, decade, dt) for fam, decade in glue_family_cases() for dt in DT_GRID]
    assert len(rec["X"]) == len(cases) == 182
    outputs = ("X", "Wx", "Wb", "dgbias")
    finite = {c: all(np.isfinite(rec[n][k]).all() for n in outputs) for k, c in enumerate(cases)}
    clean = [dt for dt in DT_GRID if all(v for (fam, _, d), v in finite.items() if d == dt and fam != "nan-entry")]
    broken = [dt for dt in DT_GRID if any(not np.isfinite(rec["Wb"][k]).all() for k, c in enumerate(cases) if c[2] == dt)]
    assert len(clean) >= 1 and len(broken) >= 3, (clean, broken)
    ctx = B.Context(B.default_params(96, 128, keylines_ref=3000, keylines_max=4000))
    n_words = 0
    for k, (fam, decade, dt) in enumerate(cases):
        g = glue_family(fam, decade)
        sides = ctx.test_glue(g["vel"], g["JtJ6"], 100.0, 1.0, 1, g["xrv"], g["n_new"], float(np.float32(dt)), g["Bg"], g["W_Bg"], g["R_prior"])
        with np.errstate(all="ignore"):
            Bg_after = (g["Bg"] + rec["dgbias"][k]).astype(np.float32)
        for side, (out, st, _) in zip(("device", "host"), sides):
            what = (side, fam, decade, dt)
            assert np.array_equal(words(out.Xv), words(rec["Xv"][k])), (what, "Xv is not the recorded input", np.array(out.Xv), rec["Xv"][k])
            assert np.array_equal(words(out.W_Xv), words(rec["W_Xv"][k])), (what, "W_Xv is not the recorded input")
            assert np.array_equal(words(out.Xgv), words(rec["X"][k])), (what, "Xgv", np.array(out.Xgv), rec["X"][k])
            assert np.array_equal(words(st[3:12]), words(rec["Wb"][k])), (what, "W_Bg", st[3:12], rec["Wb"][k])
            assert np.array_equal(words(st[:3]), words(Bg_after)), (what, "Bg", st[:3], Bg_after)
            n_words += 18 + 42
    print(f"\ndevice glue vs reference gyroBiasCorrection: {len(cases)} calls, {sum(finite.values())} with every output finite, "
          f"{n_words} words compared")
    ctx.close()
