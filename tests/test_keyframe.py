"""Keyframes without a GPU: the numpy restatement the GPU tests compare against (tests/support.py: np_kf_matches) on
hand-computed cases, and the surface - the header declares the keyframe entries, the binding lists them with matching signatures,
the library exports them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from support import F32, KF_MATCH_DTYPE, ROOT, np_kf_matches

ENTRIES = ("rebvio_hip_map_mark_keyframe", "rebvio_hip_keyframe_next", "rebvio_hip_map_keyframe_matches")


def keylines(ids, sigma, rho=None, matches=None):
    from rebvio_amd.backend import KEYLINE_DTYPE
    kl = np.zeros(len(ids), KEYLINE_DTYPE)
    kl["match_id_keyframe"] = ids
    kl["sigma_rho"] = np.asarray(sigma, F32)
    kl["rho"] = np.arange(len(ids), dtype=F32) + 1 if rho is None else rho
    kl["matches"] = np.arange(len(ids)) * 2 if matches is None else matches
    kl["pos_img"] = np.stack([np.arange(len(ids)) * 10.0, np.arange(len(ids)) * -1.0], 1).astype(F32)
    return kl


def test_smallest_sigma_wins_and_records_come_in_slot_order():
    #            keyline  0    1    2    3    4    5
    kl = keylines([3, -1, 0, 3, 0, 7], [0.5, 0.1, 0.3, 0.2, 0.4, 0.1])
    rec, count = np_kf_matches(kl, 8)
    assert count == 3 and rec.dtype == KF_MATCH_DTYPE
    assert rec["kf_keyline"].tolist() == [0, 3, 7]
    assert rec["keyline"].tolist() == [2, 3, 5]
    assert rec["claimants"].tolist() == [2, 2, 1]
    assert rec["rho"].tolist() == [3.0, 4.0, 6.0] and rec["matches"].tolist() == [4, 6, 10]
    assert rec["sigma_rho"].tolist() == [F32(0.3), F32(0.2), F32(0.1)]
    assert rec["pos_img"].tolist() == [[20.0, -2.0], [30.0, -3.0], [50.0, -5.0]]


def test_kf_size_bounds_the_slots():
    kl = keylines([0, 1, 2, 2, 3], [1, 1, 1, 1, 1])
    assert np_kf_matches(kl, 0)[1] == 0
    assert np_kf_matches(kl, 1)[0]["kf_keyline"].tolist() == [0]
    assert np_kf_matches(kl, 3)[0]["kf_keyline"].tolist() == [0, 1, 2]      # an id of kf_size is ignored
    assert np_kf_matches(kl, 4)[0]["claimants"].tolist() == [1, 1, 2, 1]
    assert np_kf_matches(keylines([-1, -5, 9], [1, 1, 1]), 9)[1] == 0


def test_the_index_breaks_ties_and_unordered_sigmas_lose():
    nan, inf = float("nan"), float("inf")
    # equal sigma_rho: the smaller index; -0.0 counts as 0.0 (so keyline 1 does not beat keyline 0 ... and would not lose to it)
    assert np_kf_matches(keylines([0, 0, 0], [0.25, 0.25, 0.5]), 1)[0]["keyline"].tolist() == [0]
    assert np_kf_matches(keylines([0, 0], [0.0, -0.0]), 1)[0]["keyline"].tolist() == [0]
    assert np_kf_matches(keylines([0, 0], [-0.0, 0.0]), 1)[0]["keyline"].tolist() == [0]
    assert np.signbit(np_kf_matches(keylines([0, 0], [-0.0, 0.0]), 1)[0]["sigma_rho"][0])    # ... stored as it is
    # NaN and negative values sort behind everything, +inf included; among themselves the index decides
    assert np_kf_matches(keylines([0, 0, 0, 0], [nan, -1.0, inf, -inf]), 1)[0]["keyline"].tolist() == [2]
    assert np_kf_matches(keylines([0, 0, 0], [nan, -1.0, -inf]), 1)[0]["keyline"].tolist() == [0]
    assert np_kf_matches(keylines([0, 0, 0], [-1.0, nan, 3.0]), 1)[0]["keyline"].tolist() == [2]
    rec, count = np_kf_matches(keylines([0] * 5, [nan] * 5), 1)
    assert count == 1 and rec["claimants"][0] == 5 and rec["keyline"][0] == 0 and np.isnan(rec["sigma_rho"][0])


def test_every_keyline_of_a_marked_map_is_its_own_correspondence():
    n = 300
    rec, count = np_kf_matches(keylines(np.arange(n), np.full(n, 20.0)), n)
    assert count == n and np.array_equal(rec["kf_keyline"], np.arange(n)) and np.array_equal(rec["keyline"], np.arange(n))
    assert (rec["claimants"] == 1).all()


# ---- the surface ---------------------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "rebvio_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_keyframe_entries():
    text = " ".join(_header().split())
    assert "int rebvio_hip_map_mark_keyframe(rebvio_hip_ctx* ctx, rebvio_hip_map* map);" in text
    assert "int rebvio_hip_keyframe_next(rebvio_hip_ctx* ctx);" in text
    assert ("int rebvio_hip_map_keyframe_matches(rebvio_hip_map* map, int kf_size, rebvio_hip_kf_match* out_host, int cap, "
            "int* count);") in text
    m = re.search(r"typedef struct rebvio_hip_kf_match \{(.*?)\} rebvio_hip_kf_match;", text)
    assert m, "rebvio_hip_kf_match"
    fields = [f.strip() for f in m.group(1).split(";") if f.strip()]
    assert fields == ["int kf_keyline", "int keyline", "int claimants", "unsigned int matches", "float rho, sigma_rho", "float pos_img[2]"]
    assert "#define REBVIO_HIP_ABI_VERSION 3" in _header()      # additions only


def test_binding_lists_the_keyframe_entries_with_matching_signatures():
    from rebvio_amd import backend as B
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    assert B.SIGNATURES["rebvio_hip_map_mark_keyframe"] == (C.c_int, [vp, vp])
    assert B.SIGNATURES["rebvio_hip_keyframe_next"] == (C.c_int, [vp])
    assert B.SIGNATURES["rebvio_hip_map_keyframe_matches"] == (C.c_int, [vp, C.c_int, C.POINTER(B.KfMatch), C.c_int, ip])
    assert C.sizeof(B.KfMatch) == 32 == B.KF_MATCH_DTYPE.itemsize and B.KF_MATCH_DTYPE == KF_MATCH_DTYPE
    # the ctypes struct and the numpy record agree field by field
    for (name, ctype), np_name in zip(B.KfMatch._fields_, B.KF_MATCH_DTYPE.names):
        assert name == np_name
        assert getattr(B.KfMatch, name).offset == B.KF_MATCH_DTYPE.fields[name][1]
        assert C.sizeof(ctype) == B.KF_MATCH_DTYPE.fields[name][0].itemsize
    for method in ("mark_keyframe", "keyframe_matches"):
        assert callable(getattr(B.Map, method))
    assert callable(B.Context.keyframe_next)


def test_library_exports_the_keyframe_entries():
    from rebvio_amd import backend as B
    if not os.path.exists(B.LIB_PATH):
        B.build()
    lib = C.CDLL(B.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    L = B.lib()
    # argument checks that need no device
    n = C.c_int(7)
    assert L.rebvio_hip_map_mark_keyframe(None, None) == -3
    assert L.rebvio_hip_keyframe_next(None) == -3
    assert L.rebvio_hip_map_keyframe_matches(None, 1, None, 0, C.byref(n)) == -3
    assert b"null map" in L.rebvio_hip_last_error()
