"""The depth hand-over between keyframe snapshots without a GPU: the surface (header, binding, exports, struct layouts, defaults, the
argument checks), the numpy restatement (tests/kf_handover_ref.py) on the hand-made 10x8 field of the alignment's tests with one
planted keyline per outcome, d rho_c / d rho against a central difference, and the library's own per-keyline statements run on the
host (rebvio_hip_test_kf_handover_host: kfp::handover_claim_term / handover_apply_term of rebvio_amd/csrc/kf_handover.hpp, the source
the kernels compile) against the restatement on an oracle-detected frame - bit for bit, since there is no sum whose order could
differ - and the purpose of it all: a successor that starts with rough depths ends closer to the truth.

A comparison between two implementations is valid only while nothing comes within GUARD of a decision (a cell edge, the min_cos gate,
a range clamp, the conflict gate) in the restatement; every comparing test asserts that first."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from kf_align_ref import GUARD, oracle_scene
from kf_fuse_ref import INT_MIN, RHO_MAX, RHO_MIN
from kf_handover_ref import COUNTS, assert_identities, counts_of, guard_min, np_kf_handover, purpose_case
from kf_pose_ref import DEFAULT_FILTER, true_motion
from support import F32, ROOT
from support import backend  # noqa: F401

ENTRIES = ("rebvio_hip_default_kf_handover_opts", "rebvio_hip_kf_snapshot_handover_depth", "rebvio_hip_test_kf_handover_host")
PURPOSE_SEED = 1            # the draw of test_handover_brings_the_successor_closer (chosen on the restatement: conflicts <= 5 % of associated)
WIDE = (0, 1e9, 1e-3, 20.0)


# ---- the surface ---------------------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "rebvio_hip.h")).read()
    return " ".join(re.sub(r"/\*.*?\*/", "", text, flags=re.S).split())


def test_header_declares_the_entries_and_the_structs():
    text = _header()
    for decl in ("void rebvio_hip_default_kf_handover_opts(rebvio_hip_ctx* ctx , rebvio_hip_kf_handover_opts* opts);",
                 "int rebvio_hip_kf_snapshot_handover_depth(rebvio_hip_kf_snapshot* dst, rebvio_hip_kf_snapshot* src, rebvio_hip_map* map, "
                 "const rebvio_hip_kf_handover_opts* opts, const double R[9], const double t[3], rebvio_hip_kf_handover* out, "
                 "int* assoc_host );"):
        assert decl in text, decl
    m = re.search(r"typedef struct rebvio_hip_kf_handover_opts \{(.*?)\} rebvio_hip_kf_handover_opts;", text)
    assert [f.strip() for f in m.group(1).split(";") if f.strip()] == ["rebvio_hip_cloud_filter kf_filter", "double min_cos", "double gate_sigma",
                                                                      "double q_abs", "int max_dist", "int reserved"]
    m = re.search(r"typedef struct rebvio_hip_kf_handover \{(.*?)\} rebvio_hip_kf_handover;", text)
    assert [f.strip() for f in m.group(1).split(";") if f.strip()] == ["int " + k for k in COUNTS]
    assert "#define REBVIO_HIP_ABI_VERSION 3" in text      # additions only


def test_binding_matches_the_structs(backend):
    B = backend
    vp, ip, dp, fp, up = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint)
    S = B.SIGNATURES
    O, H = C.POINTER(B.KfHandoverOpts), C.POINTER(B.KfHandover)
    assert S["rebvio_hip_default_kf_handover_opts"] == (None, [vp, O])
    assert S["rebvio_hip_kf_snapshot_handover_depth"] == (C.c_int, [vp, vp, vp, O, dp, dp, H, ip])
    assert S["rebvio_hip_test_kf_handover_host"] == (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, fp, up, fp, C.c_int,
                                                               fp, fp, C.c_int, ip, ip, fp, up, C.c_int, O, dp, dp, H, ip])
    assert C.sizeof(B.KfHandoverOpts) == 48 and C.sizeof(B.KfHandover) == 28
    assert [(n, getattr(B.KfHandoverOpts, n).offset) for n, _ in B.KfHandoverOpts._fields_] == [
        ("kf_filter", 0), ("min_cos", 16), ("gate_sigma", 24), ("q_abs", 32), ("max_dist", 40), ("reserved", 44)]
    assert [n for n, _ in B.KfHandover._fields_] == list(COUNTS)
    assert callable(B.KfSnapshot.handover_depth) and callable(B.default_kf_handover_opts) and callable(B.kf_handover_host)


def test_defaults(backend):
    o = backend.default_kf_handover_opts()
    assert (o.min_cos, o.gate_sigma, o.q_abs, o.max_dist, o.reserved) == (0.9, 3.0, 0.0, 40, 0)
    assert bytes(o.kf_filter) == bytes(backend.default_cloud_filter())
    o = backend.default_kf_handover_opts(gate_sigma=2.0, max_dist=3, kf_filter=dict(min_matches=7))
    assert (o.min_cos, o.gate_sigma, o.max_dist, o.kf_filter.min_matches, o.kf_filter.rho_max) == (0.9, 2.0, 3, 7, 20.0)


def test_library_exports_the_entries_and_refuses_without_a_device(backend):
    B = backend
    lib = C.CDLL(B.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    L = B.lib()
    out = B.KfHandover()
    assert L.rebvio_hip_kf_snapshot_handover_depth(None, None, None, None, None, None, C.byref(out), None) == -3
    assert "null" in L.rebvio_hip_last_error().decode()


# ---- the hand-made field -------------------------------------------------------------------------------------------------------------
HC = (100.0, 5.0, 4.0, 8, 10)      # fm, cx, cy, rows, cols
TZ = np.array([0.0, 0.0, 0.25])    # R = I, t = TZ: Y.z = 1 + rho / 4, u = kx / Y.z + 5, v = ky / Y.z + 4


def hand_case():
    """The field of tests/test_keyframe_align.py's hand case (see tests/test_keyframe_fuse.py): keyline 0 owns cell (4, 4) at distance
    0 and every unnamed cell at distance 5, keyline 1 cell (5, 8) at distance 1, keyline 2 cell (2, 2); (6, 6) is empty, (1, 1) belongs
    to keyline 3 whose unit is zero."""
    pos = np.array([[4.25, 4], [8, 6], [2, 2], [1, 1]], F32)
    unit = np.array([[1, 0], [0, 1], [0.6, 0.8], [0, 0]], F32)
    ids = np.zeros((8, 10), np.int32)
    dists = np.full((8, 10), 5, np.int32)
    for (y, x), (i, d) in {(4, 4): (0, 0), (5, 8): (1, 1), (2, 2): (2, 0), (1, 1): (3, 0)}.items():
        ids[y, x], dists[y, x] = i, d
    ids[6, 6], dists[6, 6] = -1, 0x7FFFFFFF
    return dict(pos=pos, unit=unit, ids=ids.reshape(-1), dists=dists.reshape(-1))


def dst_of(*rows):
    """a successor of len(rows) slots: (rho, sigma_rho, matches) each, pos_img = a mark that must survive"""
    p = np.array([[10.5 + k, -3.25, r[0], r[1]] for k, r in enumerate(rows)], F32).reshape(-1, 4)
    return p, np.array([r[2] for r in rows], np.uint32)


def both(backend, prs4, mt, dst, normals=None, t=TZ, flt=DEFAULT_FILTER, **kw):
    """one hand-over at R = I, t on the hand field through the restatement and the hook, asserted equal word for word; the restatement"""
    Hc = hand_case()
    prs4, mt = np.array(prs4, F32).reshape(-1, 4), np.array(mt, np.uint32)
    before = prs4.tobytes(), mt.tobytes(), dst[0].tobytes(), dst[1].tobytes()
    o = dict(min_cos=0.9, max_dist=5, gate_sigma=3.0, q_abs=0.0)
    o.update(kw)
    ref = np_kf_handover(HC, prs4, mt, normals, Hc["pos"], Hc["unit"], Hc["ids"], Hc["dists"], dst[0], dst[1], np.eye(3), t, flt, **o)
    opts = backend.default_kf_handover_opts(kf_filter=dict(zip(("min_matches", "max_rel_sigma", "rho_min", "rho_max"), flt)), **o)
    got, p2, m2, a2 = backend.kf_handover_host(*HC, 5, prs4, mt, normals, Hc["pos"], Hc["unit"], Hc["ids"], Hc["dists"], dst[0], dst[1], opts,
                                               np.eye(3), t)
    assert guard_min(ref) > GUARD, ref["guards"]
    assert counts_of(got) == counts_of(ref), (counts_of(got), counts_of(ref))
    assert np.array_equal(a2, ref["assoc"]), (a2, ref["assoc"])
    assert p2.tobytes() == ref["prs4"].tobytes() and np.array_equal(m2, ref["matches"])
    assert_identities(counts_of(got))
    assert (prs4.tobytes(), mt.tobytes(), dst[0].tobytes(), dst[1].tobytes()) == before      # src (and the caller's dst) byte-identical
    assert p2[:, :2].tobytes() == dst[0][:, :2].tobytes()                                    # pos_img is never written
    return ref


# the planted src keyline: (-1.25, 0, rho 1, sigma 0.1) at t = TZ: Y.z = 1.25, u = 4, v = 4: cell (4, 4), keyline 0;
# rho_c = 1 / 1.25 = 0.8, d = 1 / 1.5625 = 0.64, sig_c = 0.064
SRC = [-1.25, 0, 1, 0.1]
REST = ((1.0, 0.3, 1),) * 3


def test_adopted_kept_conflict(backend):
    # adopted: dst slot 0 holds 0.85 +- 0.2: dr = -0.05, bound = 9 * (0.064^2 + 0.04); 0.064 < 0.2; matches = max(2, 5)
    r = both(backend, [SRC], [5], dst_of((0.85, 0.2, 2), *REST))
    assert counts_of(r) == (1, 1, 0, 1, 1, 0, 0) and r["assoc"].tolist() == [0] and r["matches"].tolist() == [5, 1, 1, 1]
    rho_c = np.float64(F32(1.0)) / 1.25
    sig_c = (1.0 / 1.5625) * np.sqrt(np.float64(F32(0.1)) ** 2)
    assert r["rho_c"][0] == rho_c and r["sig_c"][0] == sig_c and r["d"][0] == 0.64
    assert r["prs4"][0, 2] == F32(rho_c) and r["prs4"][0, 3] == F32(sig_c)
    assert r["prs4"][0, 2] == pytest.approx(0.8, rel=1e-6) and r["prs4"][0, 3] == pytest.approx(0.064, rel=1e-6)
    assert r["prs4"][1:].tobytes() == dst_of((0.85, 0.2, 2), *REST)[0][1:].tobytes()
    # matches as the max: the slot's own count stands when it is the larger one
    assert both(backend, [SRC], [5], dst_of((0.85, 0.2, 9), *REST))["matches"].tolist() == [9, 1, 1, 1]
    # kept: the slot is the better one already (0.05 < 0.064), also at equality of the fp32 sigmas (strict <)
    for sig in (0.05, float(F32(sig_c))):
        d = dst_of((0.85, sig, 2), *REST)
        r = both(backend, [SRC], [5], d)
        assert counts_of(r) == (1, 1, 0, 1, 0, 1, 0) and r["assoc"].tolist() == [-1], sig
        assert r["prs4"].tobytes() == d[0].tobytes() and np.array_equal(r["matches"], d[1])
    # conflict: 2.0 +- 0.05 against 0.8 +- 0.064: dr^2 = 1.44 > 9 * 0.0066; all bits stay
    d = dst_of((2.0, 0.5, 2), *REST)
    assert counts_of(both(backend, [SRC], [5], d)) == (1, 1, 0, 1, 1, 0, 0)          # (a wide sigma still agrees)
    d = dst_of((2.0, 0.05, 2), *REST)
    r = both(backend, [SRC], [5], d)
    assert counts_of(r) == (1, 1, 0, 1, 0, 0, 1) and r["assoc"].tolist() == [-1]
    assert r["prs4"].tobytes() == d[0].tobytes() and np.array_equal(r["matches"], d[1])
    assert counts_of(both(backend, [SRC], [5], d, gate_sigma=20.0)) == (1, 1, 0, 1, 0, 1, 0)     # inside a wider gate: kept (0.05 < 0.064)
    # a NaN in dst is a conflict (positive test), sigma or rho
    for row in ((0.85, np.nan, 2), (np.nan, 0.2, 2)):
        d = dst_of(row, *REST)
        r = both(backend, [SRC], [5], d)
        assert counts_of(r) == (1, 1, 0, 1, 0, 0, 1) and r["assoc"].tolist() == [-1]
        assert r["prs4"].tobytes() == d[0].tobytes()


def test_out_of_range_and_not_associated(backend):
    d = dst_of((0.85, 0.2, 2), *REST)
    # low: rho = RHO_MIN itself passes the filter; rho_c = rho / (1 + rho / 4) < RHO_MIN
    r = both(backend, [[-1.0, 0, 1e-3, 1e-4]], [3], d, flt=WIDE)
    assert counts_of(r) == (1, 1, 1, 0, 0, 0, 0) and r["assoc"].tolist() == [-1] and r["rho_c"][0] < RHO_MIN
    # high: t.z = -0.25, rho 3.9: Y.z = 0.025, rho_c = 156; kx = -0.025 lands on u = 4
    r = both(backend, [[-0.025, 0, 3.9, 0.1]], [3], d, t=-TZ)
    assert counts_of(r) == (1, 1, 1, 0, 0, 0, 0) and r["assoc"].tolist() == [-1] and r["rho_c"][0] > RHO_MAX
    # a non-finite sig_c: q_abs 1e200 squares to inf
    r = both(backend, [SRC], [5], d, q_abs=1e200)
    assert counts_of(r) == (1, 1, 1, 0, 0, 0, 0) and np.isinf(r["sig_c"][0])
    assert r["prs4"].tobytes() == d[0].tobytes()
    # an owner at or beyond dst's size: cell (2, 2) is keyline 2's; a successor of 2 or 0 slots has no such keyline
    k2 = [-3.0 * 1.05, -2.0 * 1.05, 0.2, 0.01]       # Y.z = 1.05: u = 2, v = 2
    assert both(backend, [k2], [3], dst_of((0.19, 0.2, 2), *REST))["assoc"].tolist() == [2]
    for rows in (((0.19, 0.2, 2),) * 2, ()):
        r = both(backend, [k2], [3], dst_of(*rows))
        assert counts_of(r) == (1, 0, 0, 0, 0, 0, 0) and r["assoc"].tolist() == [INT_MIN], rows
    # not associated: the filter, the empty cell, max_dist, the owner's zero unit, Y.z <= 0
    for row, mt, kw in ((SRC, 1, {}), ([1.25, 2.5, 1, 0.1], 5, {}), ([-2.5, 1.25, 1, 0.1], 5, dict(max_dist=4)), ([-5, -3.75, 1, 0.1], 5, {}),
                        ([-0.025, 0, 4.1, 0.1], 5, dict(t=-TZ))):
        r = both(backend, [row], [mt], d, **kw)
        assert counts_of(r) == (1, 0, 0, 0, 0, 0, 0) and r["assoc"].tolist() == [INT_MIN], row
        assert r["prs4"].tobytes() == d[0].tobytes()


def test_two_claimants(backend):
    d = dst_of((0.85, 0.2, 2), *REST)
    # different sigma: the smaller propagated sigma wins wherever it stands; the loser gets -1 - i
    near = [-1.25 * 1.01, 0, 1, 0.1]                  # (the same cell from a slightly different pos_img: u = 3.99)
    for order in ((0.1, 0.05), (0.05, 0.1)):
        rows = [SRC[:3] + [order[0]], near[:3] + [order[1]]]
        r = both(backend, rows, [5, 7], d)
        w = int(np.argmin(order))
        assert counts_of(r) == (2, 2, 0, 1, 1, 0, 0) and r["winner"][0] == w
        assert r["assoc"].tolist() == ([0, -1] if w == 0 else [-1, 0]) and r["matches"][0] == (5, 7)[w]
        assert r["prs4"][0, 3] == F32(0.64 * np.sqrt(np.float64(F32(0.05)) ** 2))
    # equal sigma: the lower j wins
    r = both(backend, [SRC, SRC, SRC], [5, 7, 9], d)
    assert counts_of(r) == (3, 3, 0, 1, 1, 0, 0) and r["assoc"].tolist() == [0, -1, -1] and r["matches"][0] == 5
    # the winner decides alone: a loser that would have agreed does not rescue a conflicting winner
    far = [-1.25, 0, 1, 0.01]
    far[2] = 1.6                                       # Y.z = 1.4: rho_c = 1.143; lands on u = 100 * (-0.0125 / 1.4) + 5 = 4.1
    r = both(backend, [SRC, far], [5, 7], dst_of((0.85, 0.05, 2), *REST))
    assert r["winner"][0] == 1 and counts_of(r) == (2, 2, 0, 1, 0, 0, 1) and r["assoc"].tolist() == [-1, -1]


def test_identity_pose_hands_rho_over_exactly(backend):
    # t = 0, R = I: Y.z = Z.z = 1, rho_c = rho / 1, d = 1, sig_c = sqrt(s * s) = s: the fp32 bits cross unchanged
    prs4 = np.array([[-1, 0, 0.7300001, 0.0123456], [3, 1, 1.9, 0.03], [-3, -2, 0.31, 0.02]], F32)      # cells (4, 4), (5, 8), (2, 2)
    d = dst_of((0.7, 0.2, 1), (2.0, 0.2, 1), (0.3, 0.2, 1), (1.0, 0.3, 1))
    r = both(backend, prs4, [3, 4, 5], d, t=np.zeros(3))
    assert counts_of(r) == (3, 3, 0, 3, 3, 0, 0) and r["assoc"].tolist() == [0, 1, 2]
    assert r["prs4"][:3, 2:].tobytes() == prs4[:, 2:].tobytes() and r["matches"].tolist() == [3, 4, 5, 1]
    assert (r["d"] == 1.0).all()


def test_bookkeeping_on_a_mixed_snapshot(backend):
    k2 = [-3.0 * 1.05, -2.0 * 1.05, 0.2, 0.01]
    prs4 = np.array([SRC, [-1.25 * 1.01, 0, 1, 0.05], [-1.0, 0, 1e-3, 1e-4], k2, [1.25, 2.5, 1, 0.1], [5 * 1.25, 2 * 1.25, 1, 0.1]], F32)
    d = dst_of((0.85, 0.2, 2), (0.8, 0.01, 4), (5.0, 0.001, 1), (1.0, 0.3, 1))
    r = both(backend, prs4, np.full(6, 3, np.uint32), d, flt=WIDE)
    # 0 and 1 claim slot 0 (1 wins, adopted), 2 is out of range on slot 0, 3 conflicts on slot 2, 4 hits the empty cell, 5 lands on (6, 10)..
    # cell (5, 10) is outside the field's inner frame: not associated
    assert r["assoc"].tolist() == [-1, 0, -1, -3, INT_MIN, INT_MIN], r["assoc"]
    assert counts_of(r) == (6, 4, 1, 2, 1, 0, 1)
    assert r["associated"] - r["out_of_range"] - r["claimed"] == 1       # one loser


def test_the_hook_refuses_what_the_entry_refuses(backend):
    B = backend
    Hc = hand_case()
    prs4, mt = np.array([SRC], F32), np.array([5], np.uint32)
    dp, dm = dst_of((0.85, 0.2, 2), *REST)
    args = (*HC, 5, prs4, mt, None, Hc["pos"], Hc["unit"], Hc["ids"], Hc["dists"], dp, dm)
    nan_R = np.eye(3)
    nan_R[1, 2] = np.nan
    d = lambda **kw: dict(opts=B.default_kf_handover_opts(max_dist=5, **kw), R=np.eye(3), t=TZ)
    for kw, word in ((d(gate_sigma=0.0), "gate_sigma"), (d(gate_sigma=float("nan")), "gate_sigma"), (d(gate_sigma=-1.0), "gate_sigma"),
                     (d(q_abs=-1e-9), "q_abs"), (d(q_abs=float("nan")), "q_abs"), (d(min_cos=-1.01), "min_cos"), (d(min_cos=1.01), "min_cos"),
                     (d(min_cos=float("nan")), "min_cos"),
                     (dict(opts=B.default_kf_handover_opts(max_dist=-1), R=np.eye(3), t=TZ), "max_dist"),
                     (dict(opts=B.default_kf_handover_opts(max_dist=6), R=np.eye(3), t=TZ), "max_dist"), (d(reserved=1), "reserved"),
                     (d(kf_filter=dict(rho_min=0.0)), "rho_min"), (d(kf_filter=dict(rho_min=3.0, rho_max=2.0)), "rho_min > rho_max"),
                     (d(kf_filter=dict(max_rel_sigma=-1.0)), "max_rel_sigma"), (d(kf_filter=dict(rho_max=float("nan"))), "NaN"),
                     (dict(R=nan_R, t=TZ), "non-finite"), (dict(R=np.eye(3), t=[0.0, np.inf, 0.0]), "non-finite"),
                     (dict(R=None, t=TZ), "null"), (dict(R=np.eye(3), t=None), "null")):
        with pytest.raises(B.HipError) as e:
            B.kf_handover_host(*args, **kw)
        assert "error -3:" in str(e.value) and word in str(e.value), (kw, str(e.value))
    ids = Hc["ids"].copy()
    ids[17] = 4
    with pytest.raises(B.HipError, match="error -3:.*field id"):
        B.kf_handover_host(*args[:11], ids, Hc["dists"], dp, dm, R=np.eye(3), t=TZ)
    # null arrays, straight at the C entry
    L, out = B.lib(), B.KfHandover()
    fp, up, ip, dbl = C.POINTER(C.c_float), C.POINTER(C.c_uint), C.POINTER(C.c_int), C.POINTER(C.c_double)
    R, t = np.eye(3), TZ.copy()
    dp2, dm2 = dp.copy(), dm.copy()
    p = dict(prs4=prs4.ctypes.data_as(fp), mt=mt.ctypes.data_as(up), pos=Hc["pos"].ctypes.data_as(fp), unit=Hc["unit"].ctypes.data_as(fp),
             ids=Hc["ids"].ctypes.data_as(ip), dists=Hc["dists"].ctypes.data_as(ip), dp=dp2.ctypes.data_as(fp), dm=dm2.ctypes.data_as(up))

    def call(out_p=C.byref(out), dst_size=4, **null):
        q = dict(p, **{k: None for k in null})
        return L.rebvio_hip_test_kf_handover_host(100.0, 5.0, 4.0, 8, 10, 5, q["prs4"], q["mt"], None, 1, q["pos"], q["unit"], 4, q["ids"],
                                                  q["dists"], q["dp"], q["dm"], dst_size, None, R.ctypes.data_as(dbl), t.ctypes.data_as(dbl),
                                                  out_p, None)
    for k in p:
        assert call(**{k: 1}) == -3, k
    assert call(out_p=None) == -3 and call(dst_size=-1) == -3
    assert dp2.tobytes() == dp.tobytes()                                         # a refused call wrote nothing
    assert call() == 0 and out.adopted == 1                                      # (normals, options and assoc may be null)
    assert dp2.tobytes() != dp.tobytes()
    # the bounds themselves are legal
    B.kf_handover_host(*args, opts=B.default_kf_handover_opts(max_dist=0, min_cos=-1.0, q_abs=0.0), R=np.eye(3), t=TZ)
    B.kf_handover_host(*args, opts=B.default_kf_handover_opts(max_dist=5, min_cos=1.0), R=np.eye(3), t=TZ)


def test_the_per_keyline_statements_as_a_stand_alone_program(tmp_path):
    """tests/cpp/kf_handover_host_check.cpp: both passes over heap buffers of exactly the needed size, non-finite, denormal and huge
    values in every field, ids beyond the successor's size. Built plainly here; its head says how to build it with sanitizers."""
    import subprocess
    exe = str(tmp_path / "kf_handover_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rebvio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "kf_handover_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr[-2000:])


# ---- the oracle's frame --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(orc_mod):
    return oracle_scene(orc_mod)


@pytest.fixture(scope="module")
def purpose(scene):
    return purpose_case(scene, PURPOSE_SEED)


def data(scene, P, normals=True):
    return (scene["cam"], P["src_prs4"], P["src_matches"], P["src_normals"] if normals else None, scene["pos"], scene["unit"], scene["ids"],
            scene["dists"], P["dst_prs4"], P["dst_matches"])


def host(backend, scene, d, R, t, **opts):
    return backend.kf_handover_host(*d[0], scene["search_range"], *d[1:], backend.default_kf_handover_opts(**opts), R, t)


def assert_same(ref, got, what=""):
    """every output word of the hook (or the device) against the restatement's, after its guards"""
    assert guard_min(ref) > GUARD, (what, ref["guards"])
    out, prs4, mt, assoc = got
    assert counts_of(out) == counts_of(ref), (what, counts_of(out), counts_of(ref))
    assert np.array_equal(assoc, ref["assoc"]), (what, np.flatnonzero(assoc != ref["assoc"])[:8])
    assert np.asarray(prs4, F32).tobytes() == ref["prs4"].tobytes(), (what, np.flatnonzero((np.asarray(prs4) != ref["prs4"]).any(1))[:8])
    assert np.array_equal(mt, ref["matches"]), what
    assert_identities(counts_of(out))


def test_d_is_the_derivative_of_rho_c_in_rho(scene, purpose):
    """d against (rho_c(rho + h) - rho_c(rho - h)) / 2h. rho_c(rho) = rho / (Z + rho tz) with Z = Z.z, D = Z + rho tz:
    rho_c' = Z / D^2 = d, rho_c'' = -2 Z tz / D^3, rho_c''' = 6 Z tz^2 / D^4 = 6 d tz^2 / D^2. The central difference is off by
    h^2 |rho_c'''| / 6 = h^2 |d| tz^2 / D^2 (+ higher orders, a factor (h tz / D)^2 smaller) and by the rounding of the two quotients,
    2 * 2^-53 |rho_c| / 2h. rho is rounded to fp32 before it is used, so the step is a power of two the fp32 rho carries exactly:
    h = 2^-10 on rho in [0.2, 2.1] (fp32 ulp <= 2^-22). With |tz| = 0.1 and D >= 0.75 on this scene (asserted): truncation
    <= 2^-20 * 0.01 / 0.5625 |d| = 1.7e-8 |d|; rounding <= 2^-53 * 2.8 / 2^-10 = 3.2e-13 with rho_c <= 2.1 / 0.75. Bound: 2e-8 |d| + 1e-12."""
    R, t = true_motion()
    assert abs(t[2]) <= 0.1 + 1e-12
    P = purpose
    ref = np_kf_handover(*data(scene, P), R, t)
    rho = P["src_prs4"][:, 2]
    sel = np.flatnonzero((ref["assoc"] != INT_MIN) & (rho > 0.2) & (rho < 2.1))
    assert len(sel) > 1000
    h = 2.0 ** -10
    rc = []
    for sgn in (+1, -1):
        p = np.array(P["src_prs4"], F32)
        p[:, 2] = (p[:, 2].astype(np.float64) + sgn * h).astype(F32)
        assert ((p[:, 2].astype(np.float64) - rho.astype(np.float64)) == sgn * h)[sel].all()         # the step is exact in fp32
        fm = F32(scene["cam"][0])
        a = (p[:, 0] / fm).astype(F32).astype(np.float64)
        b = (p[:, 1] / fm).astype(F32).astype(np.float64)
        R9 = R.reshape(9)
        Zz = (R9[6] * a + R9[7] * b) + R9[8]
        D = Zz + p[:, 2].astype(np.float64) * t[2]
        assert (D[sel] >= 0.75).all()
        rc.append(p[:, 2].astype(np.float64) / D)
    fd = (rc[0][sel] - rc[1][sel]) / (2 * h)
    d = ref["d"][sel]
    err = np.abs(fd - d)
    print(f"d vs central difference over {len(sel)} keylines: max |fd - d| {err.max():.3g}, max |d| {np.abs(d).max():.3g}, "
          f"max err / |d| {(err / np.abs(d)).max():.3g}")
    assert (err <= 2e-8 * np.abs(d) + 1e-12).all(), (err.max(), np.abs(d).max())


@pytest.mark.parametrize("normals", [True, False])
def test_hook_against_the_restatement_bit_for_bit(backend, scene, purpose, normals):
    R, t = true_motion()
    d = data(scene, purpose, normals)
    for what, kw in (("defaults", {}), ("tight gate, q_abs", dict(gate_sigma=0.8, q_abs=0.02)),
                     ("no gradient test, short reach", dict(min_cos=-1.0, max_dist=1))):
        ref = np_kf_handover(*d, R, t, **kw)
        assert_same(ref, host(backend, scene, d, R, t, **kw), what)
        assert ref["adopted"] > 500 and (what != "tight gate, q_abs" or ref["conflicts"] > 0), (what, counts_of(ref))
    # twice: the state carries over - what was adopted is now kept (equal fp32 sigmas, strict <)
    once = np_kf_handover(*d, R, t)
    twice = np_kf_handover(*d[:8], once["prs4"], once["matches"], R, t)
    got1 = host(backend, scene, d, R, t)
    got2 = backend.kf_handover_host(*d[0], scene["search_range"], *d[1:8], got1[1], got1[2], backend.default_kf_handover_opts(), R, t)
    assert_same(twice, got2, "second hand-over")
    assert twice["adopted"] == 0 and twice["kept"] >= once["adopted"] and twice["prs4"].tobytes() == once["prs4"].tobytes()


@pytest.mark.parametrize("side", ["restatement", "hook"])
def test_handover_brings_the_successor_closer(backend, scene, purpose, side):
    """The purpose: the map's keylines take depths from a smooth scene; the successor carries them perturbed at sigma = 0.2 rho, the
    outgoing keyframe - crafted behind the true motion - at sigma = 0.05 rho, perturbed by its own sigma (seeded draws clipped at 2.5).
    One hand-over at the true motion: over the adopted slots sum (rho - rho_true)^2 falls strictly and no adopted sigma_rho grows.
    Measured (seed 1, 160x120 oracle frame): see DESIGN.md 5m."""
    R, t = true_motion()
    P = purpose
    d = data(scene, P)
    ref = np_kf_handover(*d, R, t)
    assert guard_min(ref) > GUARD, ref["guards"]
    share = ref["conflicts"] / max(ref["associated"], 1)
    assert ref["associated"] > 1000 and ref["conflicts"] <= 0.05 * ref["associated"], counts_of(ref)
    if side == "restatement":
        after = ref["prs4"]
        assoc = ref["assoc"]
    else:
        _, after, _, assoc = host(backend, scene, d, R, t)
    slots = assoc[assoc >= 0]
    assert len(slots) == ref["adopted"] and len(np.unique(slots)) == len(slots)
    before = P["dst_prs4"]
    assert (after[slots, 3] < before[slots, 3]).all()
    sq = lambda p: float(((p[slots, 2].astype(np.float64) - P["rho_true"][slots]) ** 2).sum())
    rms = lambda p: float(np.sqrt((((p[slots, 2].astype(np.float64) - P["rho_true"][slots]) / P["rho_true"][slots]) ** 2).mean()))
    print(f"{side}: counts {counts_of(ref)}; conflicts / associated {share:.4f}; sum of squared depth errors over {len(slots)} adopted slots "
          f"{sq(before):.3f} -> {sq(after):.3f}; rms relative error {rms(before):.4f} -> {rms(after):.4f}; mean sigma_rho / rho "
          f"{float((before[slots, 3] / before[slots, 2]).mean()):.4f} -> {float((after[slots, 3] / after[slots, 2]).mean()):.4f}")
    assert sq(after) < sq(before)
