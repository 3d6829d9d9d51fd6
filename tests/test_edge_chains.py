"""Edge chains and polylines without a GPU: the surface (header, ABI version, binding, exports, struct layouts, defaults, every -3
refusal), the numpy restatement (tests/edge_chains_ref.py) against hand-written cases, and the library's own per-step statements run on
the host (rebvio_hip_test_edge_chains_host / _edge_polylines_host: rebvio_amd/csrc/edge_chains.hpp, the source the kernels compile)
against the restatement on oracle-detected frames and on random link tables. Integers and record bytes: every comparison is equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import params_for
from edge_chains_ref import (CHAIN_REF_DTYPE, DEFAULT_FILTER, ENTRIES, POLYLINE_DTYPE, WIDE, assert_chains_equal, assert_polylines_equal,
                             dirty_links, keylines_with_links, links_of_sequences, np_chains, np_polylines, planted_polyline_map,
                             random_links, rounds_of, shuffled_path)
from support import CLOUD_DTYPE, F32, ROOT, np_cloud
from support import backend  # noqa: F401


# ---- the surface ---------------------------------------------------------------------------------------------------------------------
def _header(comments=False):
    text = open(os.path.join(ROOT, "include", "rebvio_hip.h")).read()
    return " ".join((text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)).split())


def test_header_declares_the_entries_and_the_structs():
    text = _header()
    for decl in ("int rebvio_hip_map_edge_chains(rebvio_hip_map* map, rebvio_hip_chain_ref* refs_host, int cap_keylines, int* order_host, "
                 "int* starts_host, int cap_chains, int* n_keylines, int* n_chains);",
                 "void rebvio_hip_default_polyline_opts(rebvio_hip_polyline_opts* o);",
                 "int rebvio_hip_map_edge_polylines(rebvio_hip_map* map, const rebvio_hip_polyline_opts* opts, const rebvio_hip_cloud_pose* pose, "
                 "rebvio_hip_cloud_point* points_host, int* refs2_host, int cap_points, rebvio_hip_polyline* lines_host, int cap_lines, "
                 "int* n_points, int* n_lines);"):
        assert decl in text, decl
    assert "typedef struct rebvio_hip_chain_ref { int head, rank, length, flags; } rebvio_hip_chain_ref;" in text
    m = re.search(r"typedef struct rebvio_hip_polyline_opts \{(.*?)\} rebvio_hip_polyline_opts;", text)
    assert [f.strip() for f in m.group(1).split(";") if f.strip()] == ["rebvio_hip_cloud_filter filter", "int min_chain_length", "int reserved"]
    m = re.search(r"typedef struct rebvio_hip_polyline \{(.*?)\} rebvio_hip_polyline;", text)
    assert [f.strip() for f in m.group(1).split(";") if f.strip()] == ["int first_point", "int points", "int head", "int flags"]
    assert "#define REBVIO_HIP_ABI_VERSION 3" in text      # additions only
    added = re.search(r"Added since, without a new version.*?\*/", _header(comments=True)).group(0)
    for name in ENTRIES + ("rebvio_hip_chain_ref", "rebvio_hip_polyline_opts", "rebvio_hip_polyline"):
        assert re.search(name + r"\b", added), name
    # the launches are documented
    assert "R = ceil(log2(keylines_max))" in _header(comments=True) and "= R + 5" in _header(comments=True) and "= R + 8" in _header(comments=True)


def test_binding_matches_the_structs(backend):
    B = backend
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    S, O, P = B.SIGNATURES, C.POINTER(B.PolylineOpts), C.POINTER(B.CloudPose)
    assert S["rebvio_hip_map_edge_chains"] == (C.c_int, [vp, vp, C.c_int, ip, ip, C.c_int, ip, ip])
    assert S["rebvio_hip_default_polyline_opts"] == (None, [O])
    assert S["rebvio_hip_map_edge_polylines"] == (C.c_int, [vp, O, P, vp, ip, C.c_int, vp, C.c_int, ip, ip])
    assert S["rebvio_hip_test_edge_chains_host"] == (C.c_int, [ip, ip, C.c_int, vp, C.c_int, ip, ip, C.c_int, ip, ip])
    assert S["rebvio_hip_test_edge_polylines_host"] == (C.c_int, [C.c_float, vp, C.c_int, O, P, vp, ip, C.c_int, vp, C.c_int, ip, ip])
    assert C.sizeof(B.PolylineOpts) == 24 and B.CHAIN_REF_DTYPE.itemsize == 16 and B.POLYLINE_DTYPE.itemsize == 16
    assert [(n, getattr(B.PolylineOpts, n).offset) for n, _ in B.PolylineOpts._fields_] == [("filter", 0), ("min_chain_length", 16), ("reserved", 20)]
    assert B.CHAIN_REF_DTYPE == CHAIN_REF_DTYPE and B.POLYLINE_DTYPE == POLYLINE_DTYPE
    assert callable(B.Map.edge_chains) and callable(B.Map.edge_polylines) and callable(B.edge_chains_host) and callable(B.edge_polylines_host)
    assert B.lib().rebvio_hip_abi_version() == 3


def test_defaults(backend):
    o = backend.default_polyline_opts()
    assert (o.min_chain_length, o.reserved) == (8, 0) and bytes(o.filter) == bytes(backend.default_cloud_filter())
    o = backend.default_polyline_opts(min_chain_length=3, filter=dict(min_matches=7))
    assert (o.min_chain_length, o.filter.min_matches, o.filter.rho_max) == (3, 7, 20.0)


def test_library_exports_the_entries(backend):
    lib = C.CDLL(backend.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name


def test_every_refusal_before_a_device_is_touched(backend):
    """-3 with a message, on the entries (no map is needed to be refused: a null map is the first of them) and on the hooks, which share
    the polyline argument check with the device entry"""
    B, L = backend, backend.lib()
    n, c = C.c_int(), C.c_int()
    assert L.rebvio_hip_map_edge_chains(None, None, 0, None, None, 0, C.byref(n), C.byref(c)) == -3
    assert "null map" in L.rebvio_hip_last_error().decode()
    assert L.rebvio_hip_map_edge_polylines(None, None, None, None, None, 0, None, 0, C.byref(n), C.byref(c)) == -3
    assert "null map" in L.rebvio_hip_last_error().decode()
    idp, idn = links_of_sequences(4, paths=[[0, 1, 2, 3]])
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    for args, word in (((ip(idp), ip(idn), -1, None, 0, None, None, 0, None, None), "negative n"),
                       ((None, ip(idn), 4, None, 0, None, None, 0, None, None), "null links"),
                       ((ip(idp), ip(idn), 4, None, -1, None, None, 0, None, None), "negative cap"),
                       ((ip(idp), ip(idn), 4, None, 0, None, None, -1, None, None), "negative cap")):
        assert L.rebvio_hip_test_edge_chains_host(*args) == -3
        assert word in L.rebvio_hip_last_error().decode(), word
    kl = keylines_with_links(B.KEYLINE_DTYPE, idp, idn)
    pts, lines = np.zeros(4, CLOUD_DTYPE), np.zeros(4, POLYLINE_DTYPE)
    nan_pose = B.cloud_pose(t=[0, np.nan, 0])

    def call(opts=None, pose=None, points=pts.ctypes.data, cap_points=4, lns=lines.ctypes.data, cap_lines=4, np_=C.byref(n), nl=C.byref(c),
             keylines=kl.ctypes.data, size=4):
        return L.rebvio_hip_test_edge_polylines_host(1.0, keylines, size, opts, pose, points, None, cap_points, lns, cap_lines, np_, nl)

    assert call() == 0 and (n.value, c.value) == (0, 0)       # (a chain of 4 is below the default min_chain_length)
    assert call(opts=B.default_polyline_opts(min_chain_length=4)) == 0 and (n.value, c.value) == (4, 1)
    for kw, word in ((dict(opts=B.default_polyline_opts(min_chain_length=0)), "min_chain_length"),
                     (dict(opts=B.default_polyline_opts(min_chain_length=-5)), "min_chain_length"),
                     (dict(opts=B.default_polyline_opts(filter=dict(rho_min=0.0))), "rho_min"),
                     (dict(opts=B.default_polyline_opts(filter=dict(rho_min=2.0, rho_max=1.0))), "rho_min > rho_max"),
                     (dict(opts=B.default_polyline_opts(filter=dict(max_rel_sigma=-1.0))), "max_rel_sigma"),
                     (dict(opts=B.default_polyline_opts(filter=dict(rho_max=float("nan")))), "NaN in the filter"),
                     (dict(pose=nan_pose), "NaN in the pose"),
                     (dict(cap_points=-1), "cap_points"), (dict(points=None), "cap_points"),
                     (dict(cap_lines=-1), "cap_lines"), (dict(lns=None), "cap_lines"),
                     (dict(np_=None), "null n_points"), (dict(nl=None), "null n_points"),
                     (dict(size=-1), "negative n"), (dict(keylines=None), "null keylines")):
        assert call(**kw) == -3, kw
        assert word in L.rebvio_hip_last_error().decode(), (word, L.rebvio_hip_last_error().decode())
    assert call(points=None, cap_points=0, lns=None, cap_lines=0) == 0      # counts only


# ---- the restatement by hand -----------------------------------------------------------------------------------------------------------
def refs_list(refs):
    return [tuple(int(v) for v in r) for r in refs]


def test_restatement_on_a_path_and_a_reversed_path():
    refs, order, starts, C_ = np_chains(*links_of_sequences(4, paths=[[0, 1, 2, 3]]))
    assert refs_list(refs) == [(0, 0, 4, 0), (0, 1, 4, 0), (0, 2, 4, 0), (0, 3, 4, 0)]
    assert list(order) == [0, 1, 2, 3] and list(starts) == [0, 4] and C_ == 1
    refs, order, starts, C_ = np_chains(*links_of_sequences(4, paths=[[3, 2, 1, 0]]))
    assert refs_list(refs) == [(3, 3, 4, 0), (3, 2, 4, 0), (3, 1, 4, 0), (3, 0, 4, 0)]
    assert list(order) == [3, 2, 1, 0] and list(starts) == [0, 4] and C_ == 1


def test_restatement_on_the_dirty_links():
    """a path, a reversed path, a 2-cycle, two claimants of one id_next, an out-of-range link, a self link"""
    refs, order, starts, C_ = np_chains(*dirty_links())
    assert refs_list(refs) == [(0, 0, 3, 0), (0, 1, 3, 0), (0, 2, 3, 0), (5, 2, 3, 0), (5, 1, 3, 0), (5, 0, 3, 0), (6, 0, 2, 1), (6, 1, 2, 1),
                               (8, 0, 1, 0), (9, 0, 2, 0), (9, 1, 2, 0), (11, 0, 1, 0)]
    assert list(order) == [0, 1, 2, 5, 4, 3, 6, 7, 8, 9, 10, 11] and list(starts) == [0, 3, 6, 8, 9, 11, 12] and C_ == 6


def test_restatement_on_a_cycle_whose_smallest_member_is_not_first():
    refs, order, starts, C_ = np_chains(*links_of_sequences(5, cycles=[[3, 1, 4]], paths=[[2, 0]]))
    assert refs_list(refs) == [(2, 1, 2, 0), (1, 0, 3, 1), (2, 0, 2, 0), (1, 2, 3, 1), (1, 1, 3, 1)]
    assert list(order) == [1, 4, 3, 2, 0] and list(starts) == [0, 3, 5] and C_ == 2


def test_restatement_of_the_polylines_by_hand(backend):
    kl, want = planted_polyline_map(backend.KEYLINE_DTYPE)
    pts, refs2, lines = np_polylines(kl, 100.0)
    assert lines.tobytes() == want.tobytes()
    kept = ([k for k in range(20) if k not in (6, 13)] + list(range(25, 37)) + list(range(38, 49)) + [k for k in range(49, 64) if k != 56])
    assert list(pts["keyline"]) == kept and len(pts) == 55
    assert [tuple(r) for r in refs2[:3]] == [(0, 0), (0, 1), (0, 2)] and tuple(refs2[18]) == (25, 0) and tuple(refs2[30]) == (37, 1)


# ---- the hooks against the restatement ----------------------------------------------------------------------------------------------------
def test_hook_on_the_hand_cases(backend):
    for name, links in (("path", links_of_sequences(4, paths=[[0, 1, 2, 3]])), ("reversed", links_of_sequences(4, paths=[[3, 2, 1, 0]])),
                        ("dirty", dirty_links()), ("cycle", links_of_sequences(5, cycles=[[3, 1, 4]], paths=[[2, 0]])),
                        ("empty", links_of_sequences(0)), ("one", links_of_sequences(1)), ("self", (np.zeros(1, np.int32), np.zeros(1, np.int32))),
                        ("shuffled", shuffled_path(300, 3)), ("one cycle", links_of_sequences(257, cycles=[list(range(257))]))):
        assert_chains_equal(backend.edge_chains_host(*links), np_chains(*links), name)


def test_hook_caps_cut_the_arrays_and_not_the_counts(backend):
    links = dirty_links()
    want = np_chains(*links)
    refs, order, starts, nk, nc = backend.edge_chains_host(*links, cap_keylines=5, cap_chains=3)
    assert (nk, nc, len(refs), len(order), len(starts)) == (12, 6, 5, 5, 3)
    assert refs.tobytes() == want[0][:5].tobytes() and np.array_equal(order, want[1][:5]) and np.array_equal(starts, want[2][:3])
    assert backend.edge_chains_host(*links, cap_keylines=0, cap_chains=0)[3:] == (12, 6)


def test_hook_on_200_random_link_tables(backend):
    rng = np.random.default_rng(20)
    cyclic = links = 0
    for k in range(200):
        n = int(rng.integers(0, 301))
        idp, idn = random_links(rng, n)
        want = np_chains(idp, idn)
        assert_chains_equal(backend.edge_chains_host(idp, idn), want, k)
        cyclic += int((want[0]["flags"] & 1).any())
        links += int((want[0]["length"] > 2).sum())
    assert cyclic > 20 and links > 2000      # the draw reaches cycles and chains of several links


@pytest.fixture(scope="module")
def oracle_maps(orc_mod):
    """the oracle's detections of stream 0: 160x120 frame 0 and 320x240 frame 1 (after frame 0: the threshold servo has run)"""
    from rebvio_amd import synth
    out = {}
    for (w, h), frame in (((160, 120), 0), ((320, 240), 1)):
        frames, cam = synth.render_stream(w, h, frame + 1)
        orc = orc_mod.Oracle(params_for(orc_mod, cam))
        for k in range(frame + 1):
            m = orc.detect_u8(frames[k], k * 50000)
        out[(w, h)] = (m.keylines(), cam)
    return out


def chain_figures(refs, starts, C_, idn, n):
    lengths = np.diff(starts)
    heads = refs["head"][refs["rank"] == 0]
    cyc = np.array([refs[h]["flags"] & 1 for h in heads])
    lcyc = np.array([refs[h]["length"] for h in heads])[cyc == 1]
    linked = int(((idn >= 0) & (idn < n)).sum())
    answered = int((lengths - 1).sum() + (cyc == 1).sum())      # a path of L members has L - 1 links, a cycle L
    return dict(keylines=n, chains_of_2_or_more=int((lengths >= 2).sum()), longest=int(lengths.max()), cyclic=int(len(lcyc)),
                longest_cycle=int(lcyc.max()) if len(lcyc) else 0, unanswered=linked - answered,
                share_in_8_or_more=float(lengths[lengths >= 8].sum()) / n)


def test_hooks_on_the_oracles_detections(backend, oracle_maps):
    """the frames whose links the feature was sized on: the 160x120 frame holds a 2-cycle and unanswered id_next links, the 320x240 frame
    long cycles; chains of 8 and more hold nearly every keyline (the default min_chain_length)"""
    for size, (kl, cam) in oracle_maps.items():
        want = np_chains(kl["id_prev"], kl["id_next"])
        fig = chain_figures(want[0], want[2], want[3], kl["id_next"], len(kl))
        print(size, fig)
        assert fig["share_in_8_or_more"] > 0.98, (size, fig)
        # the figures these frames were measured at when the feature was defined
        assert (fig["keylines"], fig["longest"], fig["cyclic"], fig["longest_cycle"], fig["unanswered"]) == {
            (160, 120): (1639, 233, 1, 2, 4), (320, 240): (8285, 502, 12, 192, 33)}[size], (size, fig)
        assert_chains_equal(backend.edge_chains_host(kl["id_prev"], kl["id_next"]), want, size)
        # detection leaves rho = 1 and matches = 0: give the keylines depths so that the filter has something to decide
        rng = np.random.default_rng(7)
        kl = kl.copy()
        kl["rho"] = rng.uniform(0.05, 3.0, len(kl)).astype(F32)
        kl["sigma_rho"] = (kl["rho"] * rng.uniform(0.0, 1.0, len(kl)).astype(F32)).astype(F32)
        kl["matches"] = rng.integers(0, 6, len(kl))
        pose = (np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]], F32), np.array([0.5, -1.25, 2.0], F32), F32(1.5))
        for flt, min_len, ps in ((DEFAULT_FILTER, 8, None), (DEFAULT_FILTER, 8, pose), (WIDE, 1, pose), (DEFAULT_FILTER, 40, None)):
            opts = backend.default_polyline_opts(min_chain_length=min_len, filter=dict(zip(("min_matches", "max_rel_sigma", "rho_min", "rho_max"), flt)))
            want_p = np_polylines(kl, cam.fm, flt, min_len, ps)
            assert len(want_p[0]) > 100 and len(want_p[2]) > 5
            assert_polylines_equal(backend.edge_polylines_host(cam.fm, kl, opts, ps), want_p, (size, flt, min_len))
    small = np_chains(oracle_maps[(160, 120)][0]["id_prev"], oracle_maps[(160, 120)][0]["id_next"])[0]
    assert 2 in small["length"][small["flags"] == 1]      # the 2-cycle


# ---- polylines -------------------------------------------------------------------------------------------------------------------------
def test_polyline_hook_on_the_planted_cases(backend):
    """a chain cut into three lines by two filter failures, a chain below min_chain_length, a fully kept cycle (closed), a cycle with one
    gap at its head (one open line) and one with a gap in the middle (two open lines: a run never wraps)"""
    kl, want_lines = planted_polyline_map(backend.KEYLINE_DTYPE)
    got = backend.edge_polylines_host(100.0, kl)
    assert_polylines_equal(got, np_polylines(kl, 100.0), "planted")
    assert got[2].tobytes() == want_lines.tobytes()
    # caps: the counts stay, first_point keeps counting every point
    pts, refs2, lines, npts, nl = backend.edge_polylines_host(100.0, kl, cap_points=20, cap_lines=5)
    assert (npts, nl, len(pts), len(lines)) == (55, 7, 20, 5)
    assert pts.tobytes() == got[0][:20].tobytes() and lines.tobytes() == want_lines[:5].tobytes() and np.array_equal(refs2, got[1][:20])


def test_with_min_chain_length_1_the_points_are_a_permutation_of_the_cloud(backend):
    rng = np.random.default_rng(11)
    idp, idn = random_links(rng, 300)
    kl = keylines_with_links(backend.KEYLINE_DTYPE, idp, idn, seed=2)
    kl["matches"] = rng.integers(0, 5, 300)
    pose = (np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F32), np.array([1, 2, 3], F32), F32(0.75))
    cloud = np_cloud(kl, 120.0, DEFAULT_FILTER, pose)
    pts, refs2, lines, npts, nl = backend.edge_polylines_host(120.0, kl, backend.default_polyline_opts(min_chain_length=1), pose)
    assert npts == len(cloud) and 50 < npts < 300
    back = np.argsort(pts["keyline"], kind="stable")
    assert pts[back].tobytes() == cloud.tobytes()
    assert int(lines["points"].sum()) == npts and np.array_equal(lines["first_point"], np.cumsum(lines["points"]) - lines["points"])


# ---- the stand-alone program ------------------------------------------------------------------------------------------------------------
def test_the_per_step_statements_as_a_stand_alone_program_under_sanitizers(tmp_path):
    """tests/cpp/edge_chains_host_check.cpp over rebvio_amd/csrc/edge_chains.hpp alone, built with AddressSanitizer and
    UndefinedBehaviorSanitizer: random and adversarial link tables in heap buffers of exactly the needed size, every outcome reached.
    A program of its own on the CPU; nothing of it is loaded into this process."""
    exe = str(tmp_path / "edge_chains_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rebvio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "edge_chains_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_rounds():
    assert [rounds_of(k) for k in (1, 2, 3, 256, 257, 16000, 65536)] == [0, 1, 2, 8, 9, 14, 16]
