"""The C-ABI shared library: builds for gfx950 without a GPU, loads, and exports every symbol include/rebvio_hip.h
declares; the product path fails loudly when there is no device (no CPU fallback)."""
import ctypes
import os
import re

import pytest

from support import backend  # noqa: F401
from support import ROOT


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "rebvio_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rebvio_hip_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_all_exported(backend):
    lib = ctypes.CDLL(backend.LIB_PATH)
    names = _declared_symbols()
    assert len(names) >= 35
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, f"declared in rebvio_hip.h but not exported: {missing}"


def test_binding_covers_header(backend):
    assert sorted(backend.SIGNATURES) == _declared_symbols()
    L = backend.lib()
    assert L.rebvio_hip_abi_version() == 3


def test_keyline_layout_is_the_reference_84_bytes(backend):
    assert backend.KEYLINE_DTYPE.itemsize == 84
    assert backend.KEYLINE_DTYPE.names == ("pos", "pos_img", "match_pos_img", "gradient", "match_gradient", "gradient_norm",
                                           "match_gradient_norm", "rho", "sigma_rho", "id", "id_prev", "id_next", "match_id",
                                           "match_id_forward", "match_id_keyframe", "matches")


def test_default_params_are_the_reference_defaults(backend):
    p = backend.default_params(480, 752)
    assert (p.keylines_ref, p.keylines_max) == (12000, 16000)           # edge_detector.hpp:20-21
    assert p.threshold == pytest.approx(0.01) and p.gain == pytest.approx(5e-7)
    assert p.search_range == 40.0 and p.iterations == 5 and p.global_min_matches_threshold == 500  # core.hpp:83-89
    assert p.match_threshold_angle == 45.0 and p.regularization_threshold == 0.5                   # edge_map.hpp:20-23
    assert p.fm == pytest.approx(0.5 * (458.654 + 457.296), rel=1e-6)                                  # camera.hpp:28


def test_create_without_gpu_fails_loudly(backend):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(backend.HipError):
        backend.Context(backend.default_params(480, 640))


def test_invalid_params_rejected(backend):
    # validated before any device is touched
    # keylines_max 65537: one more than the 256 record groups the LM reduction stages in LDS (search_range 20 keeps the
    # distance-field key bound, the only other limit on it, satisfied)
    # the first sizes outside the accepted envelope (32x32 .. 4096 columns x 2548 rows) and the first search_range past 255
    # (with a keylines_max and a match uncertainty that keep the other two limits on it satisfied)
    for kw in (dict(rows=16), dict(quantile_num_bins=500), dict(keylines_max=200000),
               dict(keylines_max=65537, search_range=20.0), dict(keylines_max=0),
               dict(cols=4097), dict(rows=2549), dict(rows=31), dict(cols=31),
               dict(search_range=256.0, keylines_max=1000, pixel_uncertainty_match=0.0)):
        p = backend.default_params(480, 640)
        for k, v in kw.items():
            setattr(p, k, v)
        with pytest.raises(backend.HipError) as e:
            backend.Context(p)
        assert "error -3:" in str(e.value), (kw, str(e.value))  # the parameter check's own code, with or without a device


def test_envelope_corners_pass_the_parameter_check(backend):
    """The corners of the accepted envelope get past validation: without a device create fails at the device query that follows it,
    not with the parameter check's -3; with one, the context exists."""
    import torch
    for rows, cols, kw in ((32, 32, {}), (2548, 4096, dict(keylines_max=65536, keylines_ref=60000)),
                           (144, 192, dict(search_range=255.0, keylines_max=2000, keylines_ref=1500, pixel_uncertainty_match=1.0))):
        p = backend.default_params(rows, cols, **kw)
        if torch.cuda.is_available():
            backend.Context(p).close()
        else:
            with pytest.raises(backend.HipError) as e:
                backend.Context(p)
            assert "error -3:" not in str(e.value), str(e.value)


def test_a_fractional_search_range_is_refused(backend):
    """rebvio_hip_create and rebvio_hip_batch_create return -3, before any device is queried, for a search_range that is no whole
    number of pixels: the field kernels walk r over [-(int)search_range, (int)search_range), the reference up to the float itself
    (core.hpp:49) - one step more (tests/test_context_geometry.py pins the difference on the oracle). Whole numbers get past
    validation: without a device create fails at the device query that follows it, not with -3."""
    import ctypes as C
    import torch
    L = backend.lib()
    kw = dict(keylines_max=2000, keylines_ref=1500)
    for sr in (7.5, 40.5, 0.5):
        p = backend.default_params(144, 192, search_range=sr, **kw)
        h = C.c_void_p()
        for rc in (L.rebvio_hip_create(C.byref(p), C.byref(h)), L.rebvio_hip_batch_create(C.byref(p), 2, C.byref(h))):
            msg = L.rebvio_hip_last_error().decode()
            assert rc == -3 and not h.value, (sr, rc, msg)
            assert "search_range" in msg and "whole number of pixels" in msg, (sr, msg)
        with pytest.raises(backend.HipError) as e:
            backend.Context(p)
        assert "error -3:" in str(e.value), (sr, str(e.value))
    for sr, more in ((7.0, {}), (255.0, dict(pixel_uncertainty_match=1.0))):
        p = backend.default_params(144, 192, search_range=sr, **kw, **more)
        if torch.cuda.is_available():
            backend.Context(p).close()
            backend.Batch(p, 2).close()
        else:
            for make in (lambda: backend.Context(p), lambda: backend.Batch(p, 2)):
                with pytest.raises(backend.HipError) as e:
                    make()
                assert "error -3:" not in str(e.value), (sr, str(e.value))


# detection parameters whose gradient gate, !(g2 < (thr * 765 * dog_threshold)^2), cannot reject a zero gradient at the lowest
# threshold the servo can reach; and non-finite or negative ones. (fields to set, words the error has to name)
_NAN = float("nan")
REFUSED_DETECTION_PARAMS = (
    (dict(threshold=0.0, dog_threshold=0.0, pos_neg_threshold=1.0, gain=0.0), ["threshold", "dog_threshold"]),
    (dict(dog_threshold=0.0), ["dog_threshold"]),
    (dict(threshold=0.0, gain=0.0), ["threshold", "dog_threshold"]),
    (dict(min_threshold=0.0, gain=5e-7), ["min_threshold", "dog_threshold"]),
    (dict(pos_neg_threshold=_NAN), ["pos_neg_threshold", "finite"]),
    (dict(dog_threshold=_NAN), ["dog_threshold", "finite"]),
    (dict(threshold=_NAN), ["threshold", "finite"]),
    (dict(gain=_NAN), ["gain", "finite"]),
    (dict(min_threshold=_NAN), ["min_threshold", "finite"]),
    (dict(max_threshold=_NAN), ["max_threshold", "finite"]),
    (dict(pos_neg_threshold=-0.1), ["pos_neg_threshold"]),
)


def test_detection_params_whose_gradient_gate_cannot_reject_a_zero_gradient_are_refused(backend):
    """rebvio_hip_create and rebvio_hip_batch_create return -3, before any device is queried, and the message names the fields.
    (On a constant frame the first of these makes every interior pixel a keyline with a NaN position - theta2 / 0 - and the
    reference's joinEdges indexes its mask with it.)"""
    import ctypes as C
    L = backend.lib()
    for kw, words in REFUSED_DETECTION_PARAMS:
        p = backend.default_params(144, 192, **kw)
        h = C.c_void_p()
        for rc in (L.rebvio_hip_create(C.byref(p), C.byref(h)), L.rebvio_hip_batch_create(C.byref(p), 2, C.byref(h))):
            msg = L.rebvio_hip_last_error().decode()
            assert rc == -3 and not h.value, (kw, rc, msg)
            assert all(w in msg for w in words), (kw, msg)
        with pytest.raises(backend.HipError) as e:
            backend.Context(p)
        assert "error -3:" in str(e.value), (kw, str(e.value))


def test_legal_detection_corners_pass_the_parameter_check(backend):
    """Small but non-zero bounds, and min_threshold > max_threshold (the servo's threshold then takes only these two values, both above
    zero), get past validation: without a device create fails at the device query that follows it, not with -3."""
    import torch
    for kw in (dict(dog_threshold=1e-3, threshold=1e-3), dict(min_threshold=0.03, max_threshold=0.02, gain=2e-6)):
        p = backend.default_params(144, 192, keylines_ref=1500, keylines_max=2000, **kw)
        if torch.cuda.is_available():
            backend.Context(p).close()
            backend.Batch(p, 2).close()
        else:
            with pytest.raises(backend.HipError) as e:
                backend.Context(p)
            assert "error -3:" not in str(e.value), str(e.value)
            with pytest.raises(backend.HipError) as e:
                backend.Batch(p, 2)
            assert "error -3:" not in str(e.value), str(e.value)


def test_oracle_refuses_the_same_detection_params(orc_mod):
    """The oracle's context creation raises for the same set instead of crashing in join_edges later."""
    for kw, _ in REFUSED_DETECTION_PARAMS:
        with pytest.raises(ValueError, match="refused"):
            orc_mod.Oracle(orc_mod.default_params(144, 192, **kw))
    for kw in (dict(dog_threshold=1e-3, threshold=1e-3), dict(min_threshold=0.03, max_threshold=0.02, gain=2e-6)):
        orc_mod.Oracle(orc_mod.default_params(144, 192, **kw))


def test_library_installs_no_signal_handlers(backend):
    """Round 1 probed a BAR mapping under a process-wide SIGSEGV/SIGBUS handler; a library inside a ROS node must not touch
    signal dispositions. The shared object does not even import the calls."""
    import subprocess
    und = subprocess.run(["nm", "-D", "--undefined-only", backend.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("sigaction", "signal", "siglongjmp", "__sigsetjmp"):
        assert not re.search(rf"\b{sym}\b", und), sym
