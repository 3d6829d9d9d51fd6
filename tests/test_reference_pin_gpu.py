"""The HIP entry points against the reference's own compiled hot path (oracle/_ref/librebvio_ref.so, see test_reference_pin.py),
without the oracle in between: detect, the distance field, directed_match, regularize and update_inverse_depth - the stages with no
sum-order freedom - over three chained 192x144 pairs, every keyline field bit for bit. The library travels with the tree; nothing is
read from the reference checkout here (the ref_mod fixture builds only where a checkout is present, and skips only when there is
neither a checkout nor a library).

The stages between the field and directed_match (rotateKeylines, minimizeVel, forwardMatch, extRotVel) run on the reference alone
and their result is uploaded into the device's maps: their sums are order-dependent on the device and test_parity_gpu holds them to
the oracle, which test_reference_pin.py holds to this library.
"""
import numpy as np
import pytest

from conftest import params_for
from support import B, ref_mod  # noqa: F401
from support import KW_TRACK, TS, assert_keylines_equal, bits_equal, half_pixel_keylines, rodrigues

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
