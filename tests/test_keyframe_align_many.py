"""Many hypotheses against one map (rebvio_hip_map_keyframe_align_many), what of it needs no GPU: the surface, the ranking
rebvio_hip_kf_align_best, the 13 starts of rebvio_hip_kf_hypotheses_around and the host hook rebvio_hip_test_kf_align_many_host on
the oracle-detected 160x120 frame of kf_align_ref.oracle_scene. The contracts:
  - the structs are laid out as the header writes them, and every refusal of the three host entries is a -3;
  - the ranking is "status 0 and inliers >= min_inliers; most inliers, then smaller cost, then lower index";
  - the 13 starts are the numpy restatement's within AROUND_VS_NP, the first one the input exactly, every R orthonormal;
  - the hook's pose is the single hook's byte for byte, and its inliers the numpy count of used terms with |e| <= huber - compared only
    where no used term of the restatement comes within GUARD of the Huber switch (or of a cell edge or the gate) at the evaluated pose;
  - multi-start from the offset the single start fails at: the winner has at least the centre hypothesis's inliers (where it lands is
    printed and reported in DESIGN.md 5l, not bounded)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from kf_align_many_ref import FAR_OFFSET, ROT_STEP, TRANS_STEP, hyp_Rt, np_around, np_inliers, py_best, results_of, seeded_guesses
from kf_align_ref import GUARD, OFFSETS, offset_guess, oracle_scene
from kf_pose_ref import pose_err, true_motion
from support import ROOT
from support import backend  # noqa: F401

ENTRIES = ("rebvio_hip_map_keyframe_align_many", "rebvio_hip_kf_align_best", "rebvio_hip_kf_hypotheses_around",
           "rebvio_hip_test_kf_align_many_host")
# |library - numpy| over R and t of the 13 starts of test_hypotheses_around_against_numpy - measured maximum 1.11e-16 (libm's sin / cos
# against numpy's and the order of the 3x3 products); the bound is 100 x that, as DESIGN.md 5i does it.
AROUND_VS_NP = 1.11e-14


# ---- the surface ---------------------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "rebvio_hip.h")).read()
    return " ".join(re.sub(r"/\*.*?\*/", "", text, flags=re.S).split())


def test_header_declares_the_entries_and_the_structs():
    text = _header()
    for decl in ("#define REBVIO_HIP_KF_HYP_MAX 64",
                 "int rebvio_hip_map_keyframe_align_many(rebvio_hip_map* map, const rebvio_hip_kf_hypothesis* hyp, int n, "
                 "const rebvio_hip_kf_align_opts* opts, rebvio_hip_kf_hyp_result* out );",
                 "int rebvio_hip_kf_align_best(const rebvio_hip_kf_hyp_result* res, int n, int min_inliers);",
                 "int rebvio_hip_kf_hypotheses_around(rebvio_hip_kf_snapshot* snap, const double R[9], const double t[3], double rot_step, "
                 "double trans_step, rebvio_hip_kf_hypothesis out[13]);"):
        assert decl in text, decl
    m = re.search(r"typedef struct rebvio_hip_kf_hypothesis \{(.*?)\} rebvio_hip_kf_hypothesis;", text)
    assert [f.strip() for f in m.group(1).split(";") if f.strip()] == ["rebvio_hip_kf_snapshot* snap", "double R0[9], t0[3]"]
    m = re.search(r"typedef struct rebvio_hip_kf_hyp_result \{(.*?)\} rebvio_hip_kf_hyp_result;", text)
    assert [f.strip() for f in m.group(1).split(";") if f.strip()] == ["rebvio_hip_kf_pose pose", "int inliers", "int reserved"]
    assert "#define REBVIO_HIP_ABI_VERSION 3" in text      # additions only


def test_binding_matches_the_structs(backend):
    B = backend
    vp, ip, dp, fp, up = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint)
    S = B.SIGNATURES
    hp, rp = C.POINTER(B.KfHypothesis), C.POINTER(B.KfHypResult)
    assert S["rebvio_hip_map_keyframe_align_many"] == (C.c_int, [vp, hp, C.c_int, C.POINTER(B.KfAlignOpts), rp])
    assert S["rebvio_hip_kf_align_best"] == (C.c_int, [rp, C.c_int, C.c_int])
    assert S["rebvio_hip_kf_hypotheses_around"] == (C.c_int, [vp, dp, dp, C.c_double, C.c_double, hp])
    assert S["rebvio_hip_test_kf_align_many_host"] == (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, fp, up, fp, C.c_int,
                                                                 fp, fp, C.c_int, ip, ip, C.POINTER(B.KfAlignOpts), dp, dp, C.c_int, rp])
    # the C layout: a pointer and twelve doubles; the pose (55 doubles, four ints) and two ints
    assert C.sizeof(B.KfHypothesis) == 104
    assert [(n, getattr(B.KfHypothesis, n).offset) for n, _ in B.KfHypothesis._fields_] == [("snap", 0), ("R0", 8), ("t0", 80)]
    assert C.sizeof(B.KfPose) == 456 and C.sizeof(B.KfHypResult) == 464
    assert [(n, getattr(B.KfHypResult, n).offset) for n, _ in B.KfHypResult._fields_] == [("pose", 0), ("inliers", 456), ("reserved", 460)]
    assert B.KF_HYP_MAX == 64
    assert callable(B.Map.keyframe_align_many) and callable(B.kf_align_best) and callable(B.kf_hypotheses_around)
    assert callable(B.kf_align_many_host) and callable(B.kf_hypothesis)


def test_library_exports_the_entries_and_refuses_without_a_device(backend):
    B = backend
    lib = C.CDLL(B.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    L = B.lib()
    err = lambda: L.rebvio_hip_last_error().decode()
    hyp, out = (B.KfHypothesis * 2)(), (B.KfHypResult * 2)()
    assert L.rebvio_hip_map_keyframe_align_many(None, hyp, 2, None, out) == -3 and "null" in err()
    # the ranking
    assert L.rebvio_hip_kf_align_best(None, 2, 0) == -3 and "null" in err()
    assert L.rebvio_hip_kf_align_best(out, 0, 0) == -3 and "n < 1" in err()
    assert L.rebvio_hip_kf_align_best(out, -1, 0) == -3
    with pytest.raises(B.HipError, match="error -3:"):
        B.kf_align_best([], 0)
    # the 13 starts
    R, t = np.eye(3).reshape(9), np.zeros(3)
    dp = C.POINTER(C.c_double)
    pR, pt = R.ctypes.data_as(dp), t.ctypes.data_as(dp)
    o13 = (B.KfHypothesis * 13)()
    assert L.rebvio_hip_kf_hypotheses_around(None, pR, pt, 0.1, 0.1, o13) == 0                   # (a null snapshot is stored as given)
    assert L.rebvio_hip_kf_hypotheses_around(None, None, pt, 0.1, 0.1, o13) == -3 and "null" in err()
    assert L.rebvio_hip_kf_hypotheses_around(None, pR, None, 0.1, 0.1, o13) == -3 and "null" in err()
    assert L.rebvio_hip_kf_hypotheses_around(None, pR, pt, 0.1, 0.1, None) == -3 and "null" in err()
    assert L.rebvio_hip_kf_hypotheses_around(None, pR, pt, -1e-300, 0.1, o13) == -3 and "negative" in err()
    assert L.rebvio_hip_kf_hypotheses_around(None, pR, pt, 0.1, -0.1, o13) == -3 and "negative" in err()
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert L.rebvio_hip_kf_hypotheses_around(None, pR, pt, bad, 0.1, o13) == -3 and "non-finite" in err()
        assert L.rebvio_hip_kf_hypotheses_around(None, pR, pt, 0.1, bad, o13) == -3 and "non-finite" in err()
        for k in (0, 8):
            Rb = R.copy()
            Rb[k] = bad
            assert L.rebvio_hip_kf_hypotheses_around(None, Rb.ctypes.data_as(dp), pt, 0.1, 0.1, o13) == -3 and "non-finite" in err()
        tb = t.copy()
        tb[2] = bad
        assert L.rebvio_hip_kf_hypotheses_around(None, pR, tb.ctypes.data_as(dp), 0.1, 0.1, o13) == -3 and "non-finite" in err()


# ---- the ranking ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,rows,min_inliers,want", [
    ("all refused: statuses", [(2, 50, 1.0), (3, 60, 1.0), (3, 0, 0.0)], 0, -1),
    ("all refused: too few inliers", [(0, 5, 1.0), (0, 9, 1.0)], 10, -1),
    ("a status-2 result with the most inliers loses", [(0, 40, 9.0), (2, 90, 1.0), (0, 41, 9.5), (3, 95, 0.5)], 0, 2),
    ("an inlier tie is broken by cost", [(0, 40, 9.0), (0, 40, 8.5), (0, 39, 1.0), (0, 40, 8.75)], 0, 1),
    ("a full tie is broken by index", [(0, 39, 1.0), (0, 40, 8.5), (0, 40, 8.5), (0, 40, 8.5)], 0, 1),
    ("inliers == min_inliers qualifies", [(0, 12, 3.0), (0, 11, 1.0)], 12, 0),
    ("one below min_inliers does not", [(0, 11, 1.0), (0, 12, 3.0), (0, 11, 0.5)], 12, 1),
    ("one below, alone", [(0, 11, 1.0)], 12, -1),
    ("a single good one", [(0, 0, 0.0)], 0, 0),
    ("a NaN cost never beats a number in a tie", [(0, 7, float("nan")), (0, 7, 2.0)], 0, 0),
])
def test_best_on_hand_written_results(backend, what, rows, min_inliers, want):
    B = backend
    res = results_of(B, rows)
    before = [bytes(r) for r in res]
    assert B.kf_align_best(res, min_inliers) == want, what
    if not any(np.isnan(c) for _, _, c in rows):
        assert py_best(rows, min_inliers) == want, what
    assert [bytes(r) for r in res] == before                      # a pure function
    # the other fields of a result do not take part
    for r in res:
        r.pose.used, r.pose.iterations, r.reserved = 77, 3, 5
        r.pose.H[0] = 1e9
    assert B.kf_align_best(res, min_inliers) == want, what


# ---- the 13 starts --------------------------------------------------------------------------------------------------------------------
def test_hypotheses_around_against_numpy(backend):
    B = backend
    worst = 0.0
    cases = [(np.eye(3), np.zeros(3), ROT_STEP, TRANS_STEP), (*true_motion(), ROT_STEP, TRANS_STEP), (*offset_guess(*FAR_OFFSET), ROT_STEP, TRANS_STEP),
             (*offset_guess(*OFFSETS[1]), 0.5, 3.0), (*true_motion(), 1e-9, 1e-9), (*true_motion(), 0.03, 0.0), (*true_motion(), 0.0, 0.12)]
    for R, t, rs, ts in cases:
        got = B.kf_hypotheses_around(None, R, t, rs, ts)
        want = np_around(R, t, rs, ts)
        assert len(got) == 13 and all(h.snap is None for h in got)
        R0, t0 = hyp_Rt(got[0])
        assert R0.tobytes() == np.asarray(R, np.float64).tobytes() and t0.tobytes() == np.asarray(t, np.float64).tobytes()
        for k, (h, (Rw, tw)) in enumerate(zip(got, want)):
            Rg, tg = hyp_Rt(h)
            worst = max(worst, np.abs(Rg - Rw).max(), np.abs(tg - tw).max())
            assert np.abs(Rg @ Rg.T - np.eye(3)).max() <= 1e-15 + np.abs(np.asarray(R) @ np.asarray(R).T - np.eye(3)).max(), k
            if k < 7:
                assert tg.tobytes() == t0.tobytes(), k            # rotations leave t alone ...
            if k == 0 or k >= 7:
                assert Rg.tobytes() == R0.tobytes(), k            # ... and translations R
            if k >= 7:
                a, s = divmod(k - 7, 2)
                others = [i for i in range(3) if i != a]
                assert (tg[others] == t0[others]).all() and tg[a] == (t0[a] - ts if s else t0[a] + ts)
    print(f"max |library - numpy| over the 13 starts: {worst:.3g}")
    assert worst <= AROUND_VS_NP


def test_hypotheses_around_orthonormal_from_an_exact_rotation(backend):
    """every R of the 13 is orthonormal to 1e-15 when the input is (here: the identity and a rotation about one axis by an angle whose
    sine and cosine are exact enough, built in numpy and checked first)"""
    B = backend
    for R in (np.eye(3), np_around(np.eye(3), np.zeros(3), 0.25, 0.0)[3][0]):
        assert np.abs(R @ R.T - np.eye(3)).max() <= 2.3e-16
        for h in B.kf_hypotheses_around(None, R, [0.1, -0.2, 0.3], ROT_STEP, TRANS_STEP):
            Rg, _ = hyp_Rt(h)
            assert np.abs(Rg @ Rg.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(Rg) - 1.0) <= 1e-15


def test_hypotheses_around_with_zero_steps_gives_13_copies(backend):
    B = backend
    R, t = offset_guess(*OFFSETS[0])
    got = B.kf_hypotheses_around(None, R, t, 0.0, 0.0)
    first = bytes(got[0])
    assert len(got) == 13 and all(bytes(h) == first for h in got)
    assert hyp_Rt(got[0])[0].tobytes() == R.tobytes() and hyp_Rt(got[0])[1].tobytes() == t.tobytes()


# ---- the host hook on the oracle's frame ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(orc_mod):
    return oracle_scene(orc_mod)


def data(scene, normals=True, n=None):
    c = scene["craft"]
    return (scene["cam"], c["prs4"][:n], c["kf_matches"][:n], c["normals"][:n] if normals else None, scene["pos"], scene["unit"], scene["ids"],
            scene["dists"])


def many(backend, scene, d, guesses, **opts):
    Rs, ts = np.array([g[0] for g in guesses]), np.array([g[1] for g in guesses])
    return backend.kf_align_many_host(*d[0], scene["search_range"], *d[1:], Rs, ts, backend.default_kf_align_opts(**opts))


def single(backend, scene, d, R0, t0, **opts):
    return backend.kf_align_host(*d[0], scene["search_range"], *d[1:], backend.default_kf_align_opts(**opts), R0, t0)[0]


def assert_inliers(d, r, what, **opts):
    """r.inliers against the numpy count at the pose r carries, under the guards"""
    kw = {("huber" if k == "huber_px" else k): v for k, v in opts.items() if k in ("huber_px", "min_cos", "max_dist")}
    inl, used, g = np_inliers(*d, np.array(r.pose.R), np.array(r.pose.t), **kw)
    assert min(g.values()) > GUARD, (what, g)
    assert (r.pose.used, r.inliers) == (used, inl), (what, r.pose.used, used, r.inliers, inl)
    assert r.reserved == 0
    return inl


@pytest.mark.parametrize("normals", [True, False])
@pytest.mark.parametrize("max_iter", [0, 8])
def test_host_hook_equals_the_single_hook_byte_for_byte(backend, scene, normals, max_iter):
    d = data(scene, normals)
    guesses = [true_motion(), *[offset_guess(*o) for o in OFFSETS], offset_guess(*FAR_OFFSET), *seeded_guesses(4, 11, *true_motion())]
    res = many(backend, scene, d, guesses, max_iter=max_iter)
    assert len(res) == len(guesses)
    for k, ((R0, t0), r) in enumerate(zip(guesses, res)):
        assert bytes(r.pose) == bytes(single(backend, scene, d, R0, t0, max_iter=max_iter)), k
        assert 0 <= r.inliers <= r.pose.used
    # a hypothesis's result does not depend on its neighbours
    alone = many(backend, scene, d, guesses[3:4], max_iter=max_iter)
    assert bytes(alone[0]) == bytes(res[3])


def test_host_hook_inliers_against_numpy(backend, scene):
    d = data(scene)
    guesses = [true_motion(), *[offset_guess(*o) for o in OFFSETS], *seeded_guesses(3, 5, *true_motion())]
    seen = set()
    for opts in (dict(max_iter=0), dict(max_iter=8), dict(max_iter=0, huber_px=0.7, min_cos=0.5, max_dist=6)):
        for k, r in enumerate(many(backend, scene, d, guesses, **opts)):
            inl = assert_inliers(d, r, (opts, k), **opts)
            seen.add(inl < r.pose.used)
    assert seen == {True, False}                                  # both all-inlier evaluations and ones with outliers are among them
    # at the crafted motion every term is an inlier; 0.02 rad off, far from all
    at_truth, off = many(backend, scene, d, [true_motion(), offset_guess(*OFFSETS[1])], max_iter=0)
    assert at_truth.inliers == at_truth.pose.used == len(d[1]) and 12 <= off.inliers < 0.9 * off.pose.used


def test_host_hook_statuses_and_sizes(backend, scene):
    B = backend
    R0, t0 = offset_guess(*OFFSETS[0])
    # size 0: status 3, pose = guess, zero sums - for min_used 0 too
    for mu in (12, 0):
        (r,) = many(B, scene, data(scene, n=0), [(R0, t0)], min_used=mu)
        assert (r.pose.status, r.pose.candidates, r.pose.used, r.pose.iterations, r.inliers) == (3, 0, 0, 0, 0)
        assert bytes(r.pose) == bytes(single(B, scene, data(scene, n=0), R0, t0, min_used=mu))
    # status 3 (11 keylines) and status 2 (nothing passes the filter, min_used 0): the single hook's bytes, inliers counted all the same
    d11 = data(scene, n=11)
    (r,) = many(B, scene, d11, [(R0, t0)])
    assert r.pose.status == 3 and bytes(r.pose) == bytes(single(B, scene, d11, R0, t0))
    assert_inliers(d11, r, "status 3")
    d64 = data(scene, n=64)
    o = dict(min_used=0, kf_filter=dict(min_matches=100))
    (r,) = many(B, scene, d64, [(R0, t0)], **o)
    assert (r.pose.status, r.pose.used, r.inliers) == (2, 0, 0) and bytes(r.pose) == bytes(single(B, scene, d64, R0, t0, **o))


def test_host_hook_refusals(backend, scene):
    B = backend
    d = data(scene, n=64)
    R, t = true_motion()
    args = (*d[0], scene["search_range"], *d[1:])
    with pytest.raises(B.HipError, match="error -3:.*n outside"):
        B.kf_align_many_host(*args, np.zeros((0, 3, 3)), np.zeros((0, 3)))
    with pytest.raises(B.HipError, match="error -3:.*n outside"):
        B.kf_align_many_host(*args, np.array([R] * 65), np.array([t] * 65))
    assert len(B.kf_align_many_host(*args, np.array([R] * 64), np.array([t] * 64))) == 64
    bad = np.array([R, R, R])
    bad[2, 1, 1] = np.nan
    with pytest.raises(B.HipError, match="error -3:.*non-finite"):
        B.kf_align_many_host(*args, bad, np.array([t] * 3))
    tb = np.array([t] * 3)
    tb[1, 0] = np.inf
    with pytest.raises(B.HipError, match="error -3:.*non-finite"):
        B.kf_align_many_host(*args, np.array([R] * 3), tb)
    for kw, word in ((dict(huber_px=0.0), "huber_px"), (dict(max_iter=33), "max_iter"), (dict(min_used=-1), "min_used"), (dict(min_cos=1.5), "min_cos"),
                     (dict(max_dist=scene["search_range"] + 1), "max_dist"), (dict(kf_filter=dict(rho_min=0.0)), "rho_min")):
        with pytest.raises(B.HipError) as e:
            B.kf_align_many_host(*args, [R], [t], B.default_kf_align_opts(**kw))
        assert "error -3:" in str(e.value) and word in str(e.value), (kw, str(e.value))
    ids = d[6].copy()
    ids[17] = len(d[4])
    with pytest.raises(B.HipError, match="error -3:.*field id"):
        B.kf_align_many_host(*args[:11], ids, d[7], [R], [t])
    # null arrays, straight at the C entry
    L = B.lib()
    fp, up, ip, dp = C.POINTER(C.c_float), C.POINTER(C.c_uint), C.POINTER(C.c_int), C.POINTER(C.c_double)
    keep = dict(prs4=np.ascontiguousarray(d[1]), mt=np.ascontiguousarray(d[2]), pos=np.ascontiguousarray(d[4]), unit=np.ascontiguousarray(d[5]),
                ids=np.ascontiguousarray(d[6], np.int32), dists=np.ascontiguousarray(d[7], np.int32), R=np.ascontiguousarray(R.reshape(9)),
                t=np.ascontiguousarray(t))
    ty = dict(prs4=fp, mt=up, pos=fp, unit=fp, ids=ip, dists=ip, R=dp, t=dp)
    p = {k: v.ctypes.data_as(ty[k]) for k, v in keep.items()}
    out = (B.KfHypResult * 1)()
    fm, cx, cy, rows, cols = d[0]

    def call(out_p=out, **null):
        q = dict(p, **{k: None for k in null})
        return L.rebvio_hip_test_kf_align_many_host(fm, cx, cy, rows, cols, scene["search_range"], q["prs4"], q["mt"], None, 64, q["pos"], q["unit"],
                                                    len(keep["pos"]), q["ids"], q["dists"], None, q["R"], q["t"], 1, out_p)
    assert call() == 0 and out[0].pose.used == 64
    for k in p:
        assert call(**{k: 1}) == -3, k
    assert call(out_p=None) == -3


# ---- multi-start --------------------------------------------------------------------------------------------------------------------
def test_multi_start_from_the_offset_the_single_start_fails_at(backend, scene):
    """0.05 rad / 0.2 units off the crafted motion, 13 starts at 0.03 / 0.12: measured here, the winner is start 7 (t.x + 0.12) with 317
    inliers of 610 used, 0.095 from the true motion; the centre (= the single start) has 133 inliers of 364 and ends 0.246 away. Nearer,
    not converged. No bound is set on the error: only that the winner has at least the centre's inliers."""
    B = backend
    d = data(scene)
    R0, t0 = offset_guess(*FAR_OFFSET)
    hyps = B.kf_hypotheses_around(None, R0, t0, ROT_STEP, TRANS_STEP)
    res = many(B, scene, d, [hyp_Rt(h) for h in hyps])
    centre = res[0]
    assert bytes(centre.pose) == bytes(single(B, scene, d, R0, t0))
    best = B.kf_align_best(res, 12)
    for k, r in enumerate(res):
        print(f"start {k:2d}: status {r.pose.status} used {r.pose.used} inliers {r.inliers} cost {r.pose.cost:.1f} "
              f"err {pose_err(r.pose.R, r.pose.t):.3g}")
    print(f"winner {best}: err {pose_err(res[best].pose.R, res[best].pose.t):.3g}; single start: err {pose_err(centre.pose.R, centre.pose.t):.3g}")
    assert best >= 0 and res[best].pose.status == 0
    assert res[best].inliers >= centre.inliers
    assert best == py_best([(r.pose.status, r.inliers, r.pose.cost) for r in res], 12)
