"""Straight segments of the edge polylines without a GPU: the surface (header, binding, exports, struct layouts, defaults, every -3
refusal), the library's own per-point statements run on the host (rebvio_hip_test_edge_segments_host: rebvio_amd/csrc/edge_segments.hpp,
the source the kernels compile) against the restatement of tests/edge_segments_ref.py by equality of record bytes and counts - on
oracle-tracked frames, on 200 random planted maps and on planted cases whose answers are stated here by hand - and two independent
statements: the fit against numpy.linalg.lstsq, and what the fit is for (the end depths of a 32-keyline 3D line)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import params_for
from edge_chains_ref import WIDE
from edge_segments_ref import (COUNT_FIELDS, ENTRIES, LINE_SEGMENT_DTYPE, LOOSE, assert_segments_equal, keylines_on_paths, np_segments, opts_of,
                               planted_cases, random_planted, seg_launches, straight, with_depths)
from support import F32, ROOT
from support import backend  # noqa: F401

POSE = (np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]], F32), np.array([0.5, -1.25, 2.0], F32), F32(1.5))
FM = 100.0


# ---- the surface ---------------------------------------------------------------------------------------------------------------------
def _header(comments=False):
    text = open(os.path.join(ROOT, "include", "rebvio_hip.h")).read()
    return " ".join((text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)).split())


def test_header_declares_the_entries_and_the_structs():
    text = _header()
    for decl in ("void rebvio_hip_default_segment_opts(rebvio_hip_segment_opts* o);",
                 "int rebvio_hip_map_edge_segments(rebvio_hip_map* map, const rebvio_hip_segment_opts* opts, const rebvio_hip_cloud_pose* pose, "
                 "rebvio_hip_line_segment* segs_host, int cap_segments, rebvio_hip_segment_counts* counts);",
                 "int rebvio_hip_test_edge_segments_host(float fm, const rebvio_hip_keyline* keylines, int n, const rebvio_hip_segment_opts* opts, "
                 "const rebvio_hip_cloud_pose* pose, rebvio_hip_line_segment* segs, int cap_segments, rebvio_hip_segment_counts* counts);"):
        assert decl in text, decl
    fields = lambda name: [f.strip() for f in re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text).group(1).split(";") if f.strip()]
    assert fields("rebvio_hip_segment_opts") == ["rebvio_hip_polyline_opts poly", "float tol", "float min_length", "int min_points", "int max_rounds"]
    assert fields("rebvio_hip_line_segment") == ["float xyz0[3], xyz1[3]", "float uv0[2], uv1[2]",
                                                 "float rho0, rho1, sigma_rho0, sigma_rho1, max_dev2, chi2", "int first_point", "int points",
                                                 "int line", "int flags"]
    assert fields("rebvio_hip_segment_counts") == ["int " + ", ".join(COUNT_FIELDS)]
    assert "#define REBVIO_HIP_ABI_VERSION 3" in text      # additions only
    added = re.search(r"Added since, without a new version.*?\*/", _header(comments=True)).group(0)
    for name in ENTRIES + ("rebvio_hip_segment_opts", "rebvio_hip_line_segment", "rebvio_hip_segment_counts"):
        assert re.search(name + r"\b", added), name
    assert "then 2 * max_rounds + 5 (k_seg_init" in _header(comments=True) and seg_launches(16) == 37      # the launches are documented


def test_binding_matches_the_structs(backend):
    B = backend
    vp = C.c_void_p
    S, O, P, N = B.SIGNATURES, C.POINTER(B.SegmentOpts), C.POINTER(B.CloudPose), C.POINTER(B.SegmentCounts)
    assert S["rebvio_hip_default_segment_opts"] == (None, [O])
    assert S["rebvio_hip_map_edge_segments"] == (C.c_int, [vp, O, P, vp, C.c_int, N])
    assert S["rebvio_hip_test_edge_segments_host"] == (C.c_int, [C.c_float, vp, C.c_int, O, P, vp, C.c_int, N])
    assert C.sizeof(B.SegmentOpts) == 40 and C.sizeof(B.SegmentCounts) == 32 and B.LINE_SEGMENT_DTYPE.itemsize == 80
    assert [(n, getattr(B.SegmentOpts, n).offset) for n, _ in B.SegmentOpts._fields_] == [("poly", 0), ("tol", 24), ("min_length", 28),
                                                                                          ("min_points", 32), ("max_rounds", 36)]
    assert tuple(n for n, _ in B.SegmentCounts._fields_) == COUNT_FIELDS
    assert B.LINE_SEGMENT_DTYPE == LINE_SEGMENT_DTYPE
    assert [B.LINE_SEGMENT_DTYPE.fields[f][1] for f in ("xyz0", "xyz1", "uv0", "uv1", "rho0", "max_dev2", "chi2", "first_point", "flags")] == [
        0, 12, 24, 32, 40, 56, 60, 64, 76]
    assert callable(B.Map.edge_segments) and callable(B.edge_segments_host) and callable(B.default_segment_opts)
    assert B.lib().rebvio_hip_abi_version() == 3


def test_profile_read_has_room_for_every_kernel_name():
    """the launch sites of the library name 86 kernels (80 without the six k_seg_*) and a few template instances of directedMatch
    under names of their own: more than the 64 backend.Context.profile_read used to read, fewer than the 128 it reads now"""
    import glob
    import inspect
    from rebvio_amd import backend as B
    names, named = set(), 0
    for path in glob.glob(os.path.join(ROOT, "rebvio_amd", "csrc", "*.hip")):
        text = open(path).read()
        names |= set(re.findall(r"RH_LAUNCH\(\s*(k_\w+)", text))
        named += len(re.findall(r"RH_LAUNCH_NAMED\(", text))
    assert {"k_seg_init", "k_seg_far", "k_seg_split", "k_seg_count", "k_seg_emit", "k_seg_fit"} <= names
    print(len(names), named)
    assert 64 < len(names) and len(names) + named <= 120, (len(names), named)      # (room left: raise the cap before this fails)
    assert "cap = 128" in inspect.getsource(B.Context.profile_read)


def test_defaults(backend):
    o = backend.default_segment_opts()
    assert (o.tol, o.min_length, o.min_points, o.max_rounds) == (1.0, 4.0, 8, 16) and bytes(o.poly) == bytes(backend.default_polyline_opts())
    o = backend.default_segment_opts(tol=0.5, poly=dict(min_chain_length=3, filter=dict(min_matches=7)))
    assert (o.tol, o.max_rounds, o.poly.min_chain_length, o.poly.filter.min_matches, o.poly.filter.rho_max) == (0.5, 16, 3, 7, 20.0)


def test_library_exports_the_entries(backend):
    lib = C.CDLL(backend.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name


def test_every_refusal_before_a_device_is_touched(backend):
    """-3 with a message, on the entry (no map is needed to be refused: a null map is the first of them) and on the hook, which shares
    the argument check with the device entry"""
    B, L = backend, backend.lib()
    cnt = B.SegmentCounts()
    assert L.rebvio_hip_map_edge_segments(None, None, None, None, 0, C.byref(cnt)) == -3
    assert "null map" in L.rebvio_hip_last_error().decode()
    kl = with_depths(keylines_on_paths(B.KEYLINE_DTYPE, [straight(9)]))
    segs = np.zeros(4, LINE_SEGMENT_DTYPE)
    nan = float("nan")

    def call(opts=None, pose=None, out=segs.ctypes.data, cap=4, counts=C.byref(cnt), keylines=kl.ctypes.data, size=9):
        return L.rebvio_hip_test_edge_segments_host(FM, keylines, size, opts, pose, out, cap, counts)

    assert call() == 0 and (cnt.kept, cnt.points, cnt.lines) == (1, 9, 1)
    D = B.default_segment_opts
    for kw, word in ((dict(opts=D(tol=-0.5)), "tol and min_length"), (dict(opts=D(tol=nan)), "tol and min_length"),
                     (dict(opts=D(min_length=-1.0)), "tol and min_length"), (dict(opts=D(min_length=nan)), "tol and min_length"),
                     (dict(opts=D(min_points=1)), "min_points"), (dict(opts=D(min_points=-3)), "min_points"),
                     (dict(opts=D(max_rounds=0)), "max_rounds"), (dict(opts=D(max_rounds=33)), "max_rounds"),
                     (dict(opts=D(poly=dict(min_chain_length=0))), "min_chain_length"),
                     (dict(opts=D(poly=dict(filter=dict(rho_min=0.0)))), "rho_min"),
                     (dict(opts=D(poly=dict(filter=dict(rho_min=2.0, rho_max=1.0)))), "rho_min > rho_max"),
                     (dict(opts=D(poly=dict(filter=dict(max_rel_sigma=-1.0)))), "max_rel_sigma"),
                     (dict(opts=D(poly=dict(filter=dict(rho_max=nan)))), "NaN in the filter"),
                     (dict(pose=B.cloud_pose(t=[0, nan, 0])), "NaN in the pose"),
                     (dict(cap=-1), "cap_segments"), (dict(out=None), "cap_segments"), (dict(counts=None), "null counts"),
                     (dict(size=-1), "negative n"), (dict(keylines=None), "null keylines")):
        assert call(**kw) == -3, kw
        assert word in L.rebvio_hip_last_error().decode(), (word, L.rebvio_hip_last_error().decode())
    assert call(opts=D(max_rounds=1)) == 0 and call(opts=D(max_rounds=32)) == 0 and call(opts=D(tol=0.0, min_length=0.0, min_points=2)) == 0
    assert call(out=None, cap=0) == 0 and cnt.kept == 1      # counts only


# ---- the planted cases, by hand ------------------------------------------------------------------------------------------------------
def run_case(B, case):
    name, kl, kw, cap = case
    got = B.edge_segments_host(FM, kl, opts_of(B, kw), POSE, cap)
    assert_segments_equal(got, np_segments(kl, FM, pose=POSE, **kw), name, cap)
    return got[0], got[1].as_dict()


def spans(segs):
    return [(int(s["first_point"]), int(s["points"])) for s in segs]


def test_hook_on_the_planted_cases_with_the_answers_by_hand(backend):
    B = backend
    cases = {c[0]: c for c in planted_cases(B.KEYLINE_DTYPE)}
    seen = set()

    def run(name):
        seen.add(name)
        return run_case(B, cases[name])

    for n in (2, 7, 8, 15, 16, 17, 33):      # a straight line is one segment, whatever it means for the 16 partials
        segs, cnt = run(f"straight {n}")
        assert spans(segs) == [(0, n)] and cnt == dict(segments_all=1, kept=1, depth_valid=1, unresolved=0, rounds_used=0, points=n,
                                                       lines=1, reserved=0), (n, cnt)
        assert tuple(segs[0]["uv0"]) == (-50.0, -20.0) and tuple(segs[0]["uv1"]) == (-50.0 + (n - 1), -20.0 + 0.5 * (n - 1))
        if n == 2:      # two points: the line through them (det = w0 w1 > 0), each end with its own keyline's depth and sigma
            kl = cases["straight 2"][1]
            assert np.allclose([segs[0]["rho0"], segs[0]["rho1"]], kl["rho"], rtol=1e-6) and segs[0]["chi2"] < 1e-6
            assert np.allclose([segs[0]["sigma_rho0"], segs[0]["sigma_rho1"]], kl["sigma_rho"], rtol=1e-6)
    segs, cnt = run("L")      # the corner (9, 0) is point 9: 9 px from the chord, exactly the vertex
    assert spans(segs) == [(0, 10), (9, 10)] and (cnt["rounds_used"], cnt["unresolved"], cnt["depth_valid"]) == (1, 0, 2)
    assert tuple(segs[0]["uv1"]) == tuple(segs[1]["uv0"]) == (9.0, 0.0) and (segs["max_dev2"] == 0).all()
    segs, cnt = run("V tie")      # points 1 and 2 tie at d2 = 4: the lower index wins, and 2 stays inside [1, 3] at 16 / 13 < 1.44
    assert spans(segs) == [(0, 2), (1, 3)] and cnt["rounds_used"] == 1 and segs[1]["max_dev2"] == F32(F32(16) / F32(13))
    segs, cnt = run("zig-zag")      # every point ends as a vertex: eight segments of two points
    assert spans(segs) == [(k, 2) for k in range(8)] and cnt["segments_all"] == 8 and cnt["unresolved"] == 0 and 3 <= cnt["rounds_used"] <= 7
    segs, cnt = run("coincident ends")      # l2 == 0: the distance from q[a]; (3, 3) is farthest, then the two other corners
    assert spans(segs) == [(0, 2), (1, 2), (2, 2), (3, 2)] and cnt["rounds_used"] == 2
    segs, cnt = run("NaN inside")      # the NaN position never splits: still one segment; its member poisons the fit
    assert spans(segs) == [(0, 20)] and cnt["rounds_used"] == 0 and cnt["depth_valid"] == 0
    assert not segs[0]["xyz0"].any() and not segs[0]["xyz1"].any() and (segs[0]["rho0"], segs[0]["sigma_rho1"]) == (0, 0)
    segs, cnt = run("inf inside")
    assert cnt["points"] == 20 and cnt["depth_valid"] < cnt["kept"]
    segs, cnt = run("sigma 0, negative, tiny")      # weights 1e12 (0 and 1e-9 clamp to 1e-6) and 2500 (|-0.02|): the fit stays finite
    assert spans(segs) == [(0, 16)] and cnt["depth_valid"] == 1 and np.isfinite(segs[0]["chi2"])
    lo, hi = sorted((float(cases["sigma 0, negative, tiny"][1]["rho"][3]), float(cases["sigma 0, negative, tiny"][1]["rho"][12])))
    assert segs[0]["sigma_rho0"] < 1e-5      # the two heavy members pin the line
    segs, cnt = run("fit leaves the clamp")      # r0 = 0.0011 - 19 / 6 < 0 < rho_min: no depth, ten zeros, the geometry stays
    assert spans(segs) == [(0, 8)] and cnt["depth_valid"] == 0 and int(segs[0]["flags"]) == 0
    assert not segs[0]["xyz0"].any() and not segs[0]["xyz1"].any() and not any(segs[0][f] for f in ("rho0", "rho1", "sigma_rho0", "sigma_rho1"))
    assert tuple(segs[0]["uv1"]) == (-43.0, -16.5)
    segs, cnt = run("exactly max_rounds")      # 17 points on an arc: 4 levels, sixteen 2-point segments
    assert spans(segs) == [(k, 2) for k in range(16)] and (cnt["rounds_used"], cnt["unresolved"]) == (4, 0)
    segs, cnt = run("one round short")      # a round fewer: eight 3-point segments, each with its 1.9 px sagitta left
    assert spans(segs) == [(2 * k, 3) for k in range(8)] and (cnt["rounds_used"], cnt["unresolved"]) == (3, 8)
    assert (segs["flags"] & 2).all() and (segs["max_dev2"] > 1.9 ** 2).all() and (segs["max_dev2"] < 2.0 ** 2).all()
    assert run("min_points met")[1]["kept"] == 1 and run("min_points missed")[1]["kept"] == 0
    assert run("min_length met")[1]["kept"] == 1 and run("min_length missed")[1]["kept"] == 0
    assert cases["min_points missed"][1].shape == (9,) and run("min_points missed")[1]["segments_all"] == 1
    segs, cnt = run("cap cut")      # 16 + 1 segments, three records
    assert len(segs) == 3 and cnt["kept"] == 17 and cnt["lines"] == 2
    segs, cnt = run("empty")
    assert len(segs) == 0 and not any(cnt.values())
    assert seen == set(cases)


def test_the_fit_agrees_with_lstsq(backend):
    """an independent statement of the fit: numpy.linalg.lstsq in float64 on equal-sigma lines, within 1e-6 relative. Another fp64
    summation order moves a sum by at most n * 2^-53 relative and the 2x2 system over t in [0, 1] is well conditioned: six orders
    of margin."""
    B = backend
    rng = np.random.default_rng(3)
    for n in (8, 15, 16, 17, 33, 100):
        kl = keylines_on_paths(B.KEYLINE_DTYPE, [straight(n, dx=0.75, dy=-0.5)], sigma=0.04)
        kl["rho"] = (1.0 + 0.3 * np.arange(n) / n + rng.normal(0, 0.04, n)).astype(F32)
        segs, cnt = B.edge_segments_host(FM, kl)
        assert cnt.kept == 1 and segs[0]["flags"] == 1
        t = np.arange(n, dtype=np.float64) / (n - 1)
        A = np.stack([np.ones(n), t], 1)
        (c0, c1), *_ = np.linalg.lstsq(A, kl["rho"].astype(np.float64), rcond=None)
        s2 = np.float64(F32(0.04)) ** 2
        cov = np.linalg.inv(A.T @ A) * s2
        res = kl["rho"].astype(np.float64) - A @ np.array([c0, c1])
        want = dict(rho0=c0, rho1=c0 + c1, sigma_rho0=math.sqrt(cov[0, 0]), sigma_rho1=math.sqrt(cov[0, 0] + 2 * cov[0, 1] + cov[1, 1]),
                    chi2=float(res @ res) / s2)
        for f, w in want.items():      # every result of the fit, 1e-6 relative (the record's fp32 rounding is 6e-8 of it)
            print(n, f, float(segs[0][f]), w, abs(float(segs[0][f]) - w) / abs(w))
            assert abs(float(segs[0][f]) - w) <= 1e-6 * abs(w), (n, f, segs[0][f], w)


def test_the_fitted_end_depths_beat_a_single_keylines(backend):
    """what the feature is for: 200 planted 3D lines of 32 keylines whose rho is drawn around the truth with its sigma_rho. The end's
    error against the end keyline's own: the median ratio is below 0.5 (for equally spaced, equal-sigma points the end variance is
    2(2n - 1) / (n(n + 1)) = 0.119 of one keyline's at n = 32, 0.35 in standard deviation), and sigma_rho0 says so within 10 %."""
    B = backend
    rng = np.random.default_rng(5)
    n, sigma = 32, 0.05
    predicted = sigma * math.sqrt(2.0 * (2 * n - 1) / (n * (n + 1)))
    assert abs(predicted / sigma - 0.345) < 1e-3
    ratios = []
    for k in range(200):
        ang = rng.uniform(0, 2 * math.pi)
        pts = straight(n, rng.uniform(-40, 40), rng.uniform(-30, 30), 1.5 * math.cos(ang), 1.5 * math.sin(ang))
        truth0, truth1 = rng.uniform(0.5, 2.0, 2)
        truth = truth0 + (truth1 - truth0) * np.arange(n) / (n - 1)      # inverse depth is affine along the image of a 3D line
        kl = keylines_on_paths(B.KEYLINE_DTYPE, [pts], sigma=sigma)
        kl["rho"] = (truth + rng.normal(0, sigma, n)).astype(F32)
        segs, cnt = B.edge_segments_host(FM, kl)
        assert cnt.kept == 1 and segs[0]["flags"] == 1 and segs[0]["points"] == n
        ratios.append(abs(float(segs[0]["rho0"]) - truth0) / abs(float(kl["rho"][0]) - truth0))
        assert abs(segs[0]["sigma_rho0"] - predicted) <= 0.1 * predicted and abs(segs[0]["sigma_rho1"] - predicted) <= 0.1 * predicted
    print("median |rho0 - truth| / |rho[a] - truth| =", float(np.median(ratios)))
    assert np.median(ratios) < 0.5


# ---- the hook against the restatement ---------------------------------------------------------------------------------------------------
def test_hook_on_200_random_planted_maps(backend):
    B = backend
    rng = np.random.default_rng(21)
    kept = split = invalid = unresolved = 0
    for k in range(200):
        kl = random_planted(B.KEYLINE_DTYPE, rng)
        kw = dict(min_chain_length=int(rng.integers(1, 9)), tol=float(rng.choice([0.0, 0.3, 0.7, 1.0, 2.5])), min_points=int(rng.integers(2, 9)),
                  min_length=float(rng.choice([0.0, 2.0, 4.0])), max_rounds=int(rng.choice([1, 2, 5, 16, 32])))
        pose = POSE if k % 2 else None
        want = np_segments(kl, FM, pose=pose, **kw)
        assert_segments_equal(B.edge_segments_host(FM, kl, opts_of(B, kw), pose), want, (k, kw))
        kept, split, unresolved = kept + want[1]["kept"], split + want[1]["rounds_used"], unresolved + want[1]["unresolved"]
        invalid += want[1]["kept"] - want[1]["depth_valid"]
    print(kept, split, invalid, unresolved)
    assert kept > 300 and split > 150 and invalid > 10 and unresolved > 50      # the draw reaches every outcome


@pytest.fixture(scope="module")
def tracked_maps(orc_mod):
    """the oracle's maps of stream 0 after tracked pairs, so that depths exist: 160x120 frame 0 and 320x240 frame 1, each as the old
    map of three pairs"""
    from rebvio_amd import synth
    out = {}
    for (w, h), frame in (((160, 120), 0), ((320, 240), 1)):
        frames, cam = synth.render_stream(w, h, frame + 4)
        orc = orc_mod.Oracle(params_for(orc_mod, cam))
        maps = [orc.detect_u8(frames[k], k * 50000) for k in range(frame + 4)]
        for k in range(frame + 3):
            orc.track_pair(maps[k], maps[k + 1])
        out[(w, h)] = (maps[frame + 3].keylines(), maps[frame].keylines(), cam)
    return out


def test_hook_on_the_oracles_tracked_maps(backend, tracked_maps):
    """tracked depths under the default options and a pose, and the detection's own geometry (every keyline kept: the wide filter) at
    the two tolerances the feature was sized on; the rounds the default max_rounds = 16 rests on"""
    B = backend
    for size, (kl, kl_frame, cam) in tracked_maps.items():
        for kw, pose in ((dict(flt=(1, 0.5, 1e-3, 20.0)), POSE), (dict(flt=WIDE, max_rounds=32), None), (dict(flt=WIDE, tol=0.7, max_rounds=32), None)):
            want = np_segments(kl, cam.fm, pose=pose, **kw)
            print(size, kw, want[1])
            assert_segments_equal(B.edge_segments_host(cam.fm, kl, opts_of(B, kw), pose), want, (size, kw))
            # (three pairs leave few keylines with two matches: a handful of segments under the depth filter, all of them without it)
            assert want[1]["kept"] > (5 if "tol" not in kw and "max_rounds" not in kw else 20), (size, kw, want[1])
            assert want[1]["unresolved"] == 0 and want[1]["rounds_used"] <= 12 and want[1]["depth_valid"] > 0
        want = np_segments(kl_frame, cam.fm, flt=WIDE, max_rounds=32)
        assert_segments_equal(B.edge_segments_host(cam.fm, kl_frame, opts_of(B, dict(flt=WIDE, max_rounds=32))), want, (size, "the frame"))
        # the rounds these frames needed when the feature was defined
        assert want[1]["rounds_used"] == {(160, 120): 7, (320, 240): 9}[size], (size, want[1])
