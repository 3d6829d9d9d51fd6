"""The depth prior from a registered depth image without a device: the ABI surface and its argument checks, the host hook
(rebvio_hip_test_depth_prior_host: the statements of rebvio_amd/csrc/depth_prior.hpp, which the kernel runs too) against the numpy
restatement of the header's definition (tests/depth_prior_ref.py) bit for bit, planted cases worked out by hand, and what the prior
buys on the CPU oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import depth_prior_ref as R
from conftest import params_for
from support import KW_TRACK, backend  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
NAN = F32(np.nan)
# Statistic A of test_value_on_the_oracle as measured with this restatement on the 192x144 stream; the bound on it is
# twice this and absorbs nothing but changes of the synthetic scene.
A_MEASURED = 0.002742


def fresh(B, n, rho=1.0, sigma=20.0):
    kl = np.zeros(n, B.KEYLINE_DTYPE)
    kl["rho"], kl["sigma_rho"] = F32(rho), F32(sigma)
    kl["gradient"] = (1.0, 0.0)
    kl["gradient_norm"] = 1.0
    return kl


def both(B, rows, cols, kl, img, fmt=None, **opts):
    """the hook and the restatement on the same input, asserted equal in every word; -> (counts tuple, keylines, outcome)"""
    c, k2, oc = B.depth_prior_host(rows, cols, kl, img, fmt, B.default_depth_prior_opts(**opts) if opts else None)
    c2, k3, oc2 = R.depth_prior(kl, img, fmt, **opts)
    assert c.as_tuple() == R.counts_tuple(c2), (c.as_tuple(), R.counts_tuple(c2))
    assert np.array_equal(oc, oc2), np.flatnonzero(oc != oc2)[:8]
    for f in kl.dtype.names:
        a, b = k2[f].view(np.uint32), k3[f].view(np.uint32)
        assert np.array_equal(a, b), (f, np.flatnonzero((a != b).reshape(len(kl), -1).any(1))[:8])
    for f in kl.dtype.names:  # nothing but rho and sigma_rho moves
        if f not in ("rho", "sigma_rho"):
            assert np.array_equal(k2[f].view(np.uint32), np.ascontiguousarray(kl[f]).view(np.uint32)), f
    still = (oc & 3) != 1
    assert np.array_equal(k2["rho"][still].view(np.uint32), kl["rho"][still].view(np.uint32))
    assert np.array_equal(k2["sigma_rho"][still].view(np.uint32), kl["sigma_rho"][still].view(np.uint32))
    assert c.candidates == len(kl) and c.sampled == c.fused + c.gated
    return c.as_tuple(), k2, oc


# ---- the ABI surface --------------------------------------------------------------------------------------------------------------
def test_defaults_and_layout(backend):
    B = backend
    o = B.default_depth_prior_opts()
    assert (o.tap_px, o.jump_rel, o.z_min, o.z_max, o.sigma_z0, o.sigma_z2, o.gate_sigma, o.q_abs, o.unit, o.reserved) == \
        (2.0, 0.1, 0.1, 20.0, 1e-3, 2e-3, 3.0, 0.0, 0.001, 0)
    assert C.sizeof(B.DepthPriorOpts) == 80 and C.sizeof(B.DepthPriorCounts) == 24
    assert (B.DEPTH_U16, B.DEPTH_F32) == (0, 1)
    assert {k: getattr(o, k) for k in R.DEFAULTS} == R.DEFAULTS


BAD_OPTS = (dict(tap_px=-1.0), dict(tap_px=float("nan")), dict(tap_px=float("inf")), dict(jump_rel=-0.1), dict(jump_rel=float("nan")),
            dict(z_min=0.0), dict(z_min=float("nan")), dict(z_max=0.05), dict(z_max=float("nan")), dict(sigma_z0=-1e-3),
            dict(sigma_z2=-1e-3), dict(sigma_z0=0.0, sigma_z2=0.0), dict(sigma_z0=float("nan")), dict(gate_sigma=0.0),
            dict(gate_sigma=float("nan")), dict(q_abs=-1.0), dict(q_abs=float("nan")), dict(unit=0.0), dict(unit=float("nan")),
            dict(reserved=1))


def test_every_refusal_is_minus_3_before_a_device_is_touched(backend):
    B = backend
    L = B.lib()
    kl = fresh(B, 4)
    kl["pos"] = 8.0
    img = np.full((32, 32), 2.0, F32)
    img16 = np.full((32, 32), 2000, np.uint16)
    cnt = B.DepthPriorCounts()

    def hook(rows=32, cols=32, k=kl, n=4, depth=img, pitch=32 * 4, fmt=B.DEPTH_F32, opts=None, counts=cnt):
        return L.rebvio_hip_test_depth_prior_host(rows, cols, k.ctypes.data if k is not None else None, n,
                                                  depth.ctypes.data if depth is not None else None, pitch, fmt, opts,
                                                  C.byref(counts) if counts is not None else None, None)
    assert hook() == 0 and cnt.fused == 4
    assert hook(pitch=0) == 0            # 0 = dense
    for kw in BAD_OPTS:
        assert hook(opts=B.default_depth_prior_opts(**kw)) == -3, kw
        assert L.rebvio_hip_last_error().decode().startswith("test_depth_prior_host"), kw
    assert hook(fmt=2) == -3 and hook(fmt=-1) == -3
    assert hook(pitch=32 * 4 - 4) == -3 and hook(pitch=32 * 4 + 2) == -3      # below a row, no multiple of a tap
    assert hook(depth=img16, pitch=65, fmt=B.DEPTH_U16) == -3 and hook(depth=img16, pitch=64, fmt=B.DEPTH_U16) == 0
    assert hook(depth=None) == -3 and hook(counts=None) == -3 and hook(n=-1) == -3 and hook(k=None) == -3
    assert hook(rows=-1) == -3
    raw = np.zeros(32 * 32 * 4 + 8, np.uint8)
    off = (-raw.ctypes.data) % 4 + 1  # an address that is no multiple of 4
    assert L.rebvio_hip_test_depth_prior_host(32, 32, kl.ctypes.data, 4, raw.ctypes.data + off, 0, B.DEPTH_F32, None, C.byref(cnt), None) == -3
    # the device entries refuse a null handle before anything else
    assert L.rebvio_hip_map_fuse_depth_image(None, img.ctypes.data, 0, B.DEPTH_F32, None, C.byref(cnt), None) == -3
    assert L.rebvio_hip_map_fuse_depth_image_device(None, img.ctypes.data, 0, B.DEPTH_F32, None, C.byref(cnt), None) == -3
    assert L.rebvio_hip_map_fuse_depth_image_async(None, None, img.ctypes.data, 0, B.DEPTH_F32, None) == -3
    assert L.rebvio_hip_depth_prior_last_counts(None, C.byref(cnt)) == -3


# ---- the hook against the restatement -----------------------------------------------------------------------------------------------
def test_hook_equals_restatement_on_the_oracles_160x120_frames(backend):
    from rebvio_amd import synth
    gold = np.load(os.path.join(HERE, "golden", "pair_160x120.npz"))
    depth = synth.render_stream_depth(160, 120, 2)
    for kl, d in ((gold["det0_keylines"], depth[0]), (gold["pair1_new_keylines"], depth[1])):
        c, _, _ = both(backend, 120, 160, kl, d)
        assert c[2] > 0.8 * len(kl) and c[4] > 0, c                    # most keylines take a depth; some sit on a jump
        d16 = np.rint(d.astype(np.float64) * 1000).astype(np.uint16)
        c16, _, _ = both(backend, 120, 160, kl, d16)
        assert c16[1] == c[1]


def random_case(B, rng, it):
    rows, cols = (32, 32) if it % 2 else (33, 37)
    n = int(rng.integers(0, 300))
    kl = np.zeros(n, B.KEYLINE_DTYPE)
    kl["pos"] = rng.uniform(-3, max(rows, cols) + 3, (n, 2)).astype(F32)
    kl["gradient"] = rng.normal(0, 5, (n, 2)).astype(F32)
    kl["gradient_norm"] = np.sqrt((kl["gradient"].astype(np.float64) ** 2).sum(1)).astype(F32)
    kl["rho"] = rng.uniform(0.001, 3, n).astype(F32)
    kl["sigma_rho"] = rng.uniform(0, 2, n).astype(F32)
    kl["matches"] = rng.integers(0, 9, n)
    if (it // 2) % 2:  # pitch > width: a column slice of a wider array
        img = rng.uniform(0, 25, (rows, cols + 5)).astype(F32)[:, :cols]
        img[rng.uniform(size=img.shape) < 0.05] = NAN
    else:
        img = rng.integers(0, 25000, (rows, cols + 3)).astype(np.uint16)[:, :cols]
        img[rng.uniform(size=img.shape) < 0.1] = 0
    return rows, cols, kl, img


def test_hook_equals_restatement_on_200_random_tables(backend):
    rng = np.random.default_rng(20)
    seen = np.zeros(6, np.int64)
    for it in range(200):
        rows, cols, kl, img = random_case(backend, rng, it)
        assert img.strides[0] > cols * img.itemsize
        opts = {} if it % 5 else dict(tap_px=float(rng.uniform(0, 4)), jump_rel=float(rng.uniform(0, 1)), q_abs=float(rng.uniform(0, 1)))
        c, _, _ = both(backend, rows, cols, kl, img, **opts)
        seen += c
    assert (seen[1:5] > 500).all(), seen  # sampled, fused, gated and jumps all occur in numbers


# ---- planted cases, outcomes worked out by hand -----------------------------------------------------------------------------------
def test_taps_on_each_border_and_just_outside(backend):
    B = backend
    rows, cols = 33, 37
    img = np.full((rows, cols), 2.0, F32)
    img[:, 0] = img[:, cols - 1] = 1.0
    img[0, :] = img[rows - 1, :] = 1.0
    kl = fresh(B, 8)
    # a side tap 2 px along the gradient lands ON the border column / row (z = 1: a jump, outcome 1 + 16) ...
    kl["pos"][0], kl["gradient"][0] = (2.0, 10.0), (-1.0, 0.0)            # x = 0
    kl["pos"][1], kl["gradient"][1] = (cols - 3.0, 10.0), (1.0, 0.0)      # x = cols - 1
    kl["pos"][2], kl["gradient"][2] = (10.0, 2.0), (0.0, -1.0)            # y = 0
    kl["pos"][3], kl["gradient"][3] = (10.0, rows - 3.0), (0.0, 1.0)      # y = rows - 1
    # ... or half a pixel further, where x + 0.5 < 0 or >= cols: the tap does not exist, the other two see z = 2
    kl["pos"][4], kl["gradient"][4] = (1.25, 10.0), (-1.0, 0.0)           # x = -0.75
    kl["pos"][5], kl["gradient"][5] = (cols - 2.5, 10.0), (1.0, 0.0)      # x = cols - 0.5
    kl["pos"][6], kl["gradient"][6] = (10.0, 1.25), (0.0, -1.0)
    kl["pos"][7], kl["gradient"][7] = (10.0, rows - 2.5), (0.0, 1.0)
    c, k2, oc = both(B, rows, cols, kl, img)
    assert list(oc) == [17, 17, 17, 17, 1, 1, 1, 1] and c == (8, 8, 8, 0, 4, 0)
    # x + 0.5 == 0 exactly is inside (pixel 0), and a centre tap outside leaves the two side taps
    kl = fresh(B, 2)
    kl["pos"][0], kl["gradient"][0] = (1.5, 10.0), (-1.0, 0.0)            # x = -0.5
    kl["pos"][1], kl["gradient"][1] = (-1.0, 10.0), (1.0, 0.0)            # centre outside, x = 1 inside, x = -3 outside
    c, _, oc = both(B, rows, cols, kl, img)
    assert list(oc) == [17, 1]


def test_no_direction_uses_the_centre_tap_alone(backend):
    B = backend
    img = np.full((32, 32), 2.0, F32)
    img[10, 12] = img[10, 8] = 1.0  # where the side taps of (10, 10) along x would land
    kl = fresh(B, 5)
    kl["pos"] = (10.0, 10.0)
    kl["gradient_norm"] = (1.0, 0.0, NAN, -1.0, 1.0)
    kl["gradient"][4] = (np.inf, 0.0)  # a quotient that is not finite
    c, _, oc = both(B, 32, 32, kl, img)
    assert list(oc) == [17, 1, 1, 1, 1]


def test_bad_positions_and_invalid_taps_give_no_depth(backend):
    B = backend
    img = np.full((32, 32), 2.0, F32)
    kl = fresh(B, 4, rho=0.7, sigma=0.3)
    kl["pos"] = ((NAN, 5.0), (5.0, np.inf), (-np.inf, NAN), (1e30, 5.0))
    c, k2, oc = both(B, 32, 32, kl, img)
    assert list(oc) == [0, 0, 0, 0] and c == (4, 0, 0, 0, 0, 0)
    kl = fresh(B, 1)
    kl["pos"] = (10.0, 10.0)
    for bad in (0.05, 25.0, np.nan, np.inf, -2.0, 0.0):  # below z_min, above z_max, and what fails both positive tests
        c, _, oc = both(B, 32, 32, kl, np.full((32, 32), bad, F32))
        assert list(oc) == [0], bad
    for bad in (0, 99, 20001):  # u16: invalid, 0.099 m, 20.001 m
        c, _, oc = both(B, 32, 32, kl, np.full((32, 32), bad, np.uint16))
        assert list(oc) == [0], bad
    # u16 value 0 at the centre alone: the side taps carry the keyline; z bounds are inclusive
    img = np.full((32, 32), 2000, np.uint16)
    img[10, 10] = 0
    assert list(both(B, 32, 32, kl, img)[2]) == [1]
    assert list(both(B, 32, 32, kl, np.full((32, 32), 100, np.uint16))[2]) == [1]
    assert list(both(B, 32, 32, kl, np.full((32, 32), 20000, np.uint16))[2]) == [1]
    # unit: 2000 counts of 0.5 mm are 1 m
    _, k2, _ = both(B, 32, 32, kl, np.full((32, 32), 2000, np.uint16), unit=0.0005)
    assert abs(float(k2["rho"][0]) - 1.0) < 1e-6


def test_jump_exactly_at_and_one_ulp_over(backend):
    B = backend
    kl = fresh(B, 2, rho=0.5)
    kl["pos"] = ((10.0, 10.0), (10.0, 20.0))
    img = np.full((32, 32), 2.0, F32)
    img[10, 12] = 3.0                          # 3 - 2 = 1 = 0.5 * 2: not a jump
    img[20, 12] = np.nextafter(F32(3.0), F32(4.0))  # one ulp more: a jump
    c, _, oc = both(B, 32, 32, kl, img, jump_rel=0.5)
    assert list(oc) == [1, 17] and c[4] == 1


def test_innovation_exactly_at_the_gate(backend):
    B = backend
    # v = 0 (sigma_rho 0, q_abs 0): S = s_m^2 = 0.25^2, gate 2: fused while e^2 <= 0.25. z = 2: rho_m = 0.5
    kl = fresh(B, 3, sigma=0.0)
    kl["pos"] = (10.0, 10.0)
    kl["rho"] = (1.0, np.nextafter(F32(1.0), F32(2.0)), 0.25)
    c, k2, oc = both(B, 32, 32, kl, np.full((32, 32), 2.0, F32), sigma_z0=0.0, sigma_z2=0.25, gate_sigma=2.0)
    assert list(oc) == [1, 2, 1] and c == (3, 3, 2, 1, 0, 0)
    assert np.array_equal(k2["rho"].view(np.uint32), kl["rho"].view(np.uint32))  # K = 0: the fused ones keep their value
    assert list(k2["sigma_rho"]) == [0.0, 0.0, 0.0]


def test_fresh_keylines_take_the_sensors_depth(backend):
    B = backend
    kl = fresh(B, 3)
    kl["pos"] = ((5.0, 5.0), (15.0, 5.0), (25.0, 5.0))
    img = np.full((32, 32), 2.0, F32)
    img[:, 10:20] = 4.0
    img[:, 20:] = 0.8
    c, k2, oc = both(B, 32, 32, kl, img, tap_px=0.0)
    assert list(oc) == [1, 1, 1]
    for i, z in enumerate((2.0, 4.0, 0.8)):
        rho_m = 1.0 / np.float64(F32(z))
        s_m = 1e-3 * rho_m * rho_m + 2e-3
        K = 400.0 / (400.0 + s_m * s_m)
        assert abs(float(k2["rho"][i]) - rho_m) <= (1 - K) * abs(rho_m - 1.0) + 2.0 ** -24 * rho_m, (i, k2["rho"][i])
        assert abs(float(k2["sigma_rho"][i]) - s_m) <= 1e-6 * s_m, (i, k2["sigma_rho"][i])   # sqrt((1 - K) * 400) ~ s_m
    assert np.array_equal(k2["matches"], kl["matches"])


def test_both_clamps(backend):
    B = backend
    kl = fresh(B, 2)
    kl["pos"] = ((5.0, 5.0), (25.0, 5.0))
    img = np.full((32, 32), 0.04, F32)  # rho_m = 25 > RHO_MAX
    img[:, 16:] = 2000.0                # rho_m = 5e-4 < RHO_MIN
    c, k2, oc = both(B, 32, 32, kl, img, z_min=0.01, z_max=5000.0, tap_px=0.0)
    assert list(oc) == [33, 33] and c == (2, 2, 2, 0, 0, 2)
    assert k2["rho"][0] == F32(20.0) and k2["rho"][1] == F32(1e-3)
    s_m = 1e-3 * 5e-4 * 5e-4 + 2e-3
    assert abs(float(k2["sigma_rho"][1]) - (s_m + (1e-3 - 5e-4))) < 1e-6   # the overshoot is added to sigma_rho


def test_sigma_rho_zero(backend):
    B = backend
    kl = fresh(B, 2, rho=0.5, sigma=0.0)
    kl["pos"] = (10.0, 10.0)
    kl["rho"][1] = 0.6
    c, k2, oc = both(B, 32, 32, kl, np.full((32, 32), 2.0, F32))
    assert list(oc) == [1, 2]  # a certain keyline that agrees stays as it is; one that disagrees by 0.1 >> 3 s_m is gated
    assert list(k2["rho"]) == [F32(0.5), F32(0.6)] and list(k2["sigma_rho"]) == [0.0, 0.0]
    c, k2, oc = both(B, 32, 32, kl, np.full((32, 32), 2.0, F32), q_abs=1.0)  # q_abs reopens it
    assert list(oc) == [1, 1] and abs(float(k2["rho"][1]) - 0.5) < 1e-5


def test_empty_table(backend):
    c, k2, oc = both(backend, 32, 32, np.zeros(0, backend.KEYLINE_DTYPE), np.full((32, 32), 2.0, F32))
    assert c == (0, 0, 0, 0, 0, 0) and len(k2) == 0 and len(oc) == 0


# ---- what it buys -------------------------------------------------------------------------------------------------------------------
def test_value_on_the_oracle(orc_mod, small_stream):
    """The 192x144 KW_TRACK stream, 10 frames, on the CPU oracle in device sum order; the restatement fuses the rendered, noise-free
    depth image of frame k into map k after its pair (map 0: after detection). A = the median over frames 2..9 of the median
    relative depth error |1 / rho - z_near| / z_near of the default-cloud-filter keylines, taken before that frame's own fusion;
    B = the same without depth. Measured: A = 0.002742, B = 0.5633; |V| 0.0208 - 0.0222 against the scene's 0.0229 m per frame
    (0.0139 - 0.0146, scale-free, without depth); 1835 - 1946 keylines pass the filter against 809 - 1482."""
    from rebvio_amd import synth
    frames, cam = small_stream
    frames = frames[:10]
    depth = synth.render_stream_depth(cam.width, cam.height, 10)
    p = params_for(orc_mod, cam, **KW_TRACK)
    a = R.oracle_stream(orc_mod, p, frames, depth, True)
    b = R.oracle_stream(orc_mod, p, frames, depth, False)
    A, Bv = float(np.median(a["err"][2:])), float(np.median(b["err"][2:]))
    v_a = [float(np.linalg.norm(r.V)) for r in a["records"]]
    v_b = [float(np.linalg.norm(r.V)) for r in b["records"]]
    print(f"A = {A:.6f}  B = {Bv:.6f}  |V| with depth {min(v_a):.4f}..{max(v_a):.4f}  without {min(v_b):.4f}..{max(v_b):.4f}  "
          f"passing {a['passing'][2:]} against {b['passing'][2:]}")
    assert all(r.status == 0 for r in a["records"]) and all(r.status == 0 for r in b["records"])
    assert A <= Bv / 10, (A, Bv)
    assert A <= 2 * A_MEASURED, (A, A_MEASURED)
