"""The lookup through a map's distance field (kfp::lookup of rebvio_amd/csrc/kf_pose.hpp: project, cell, owner, gradient-direction
test) is one statement with three consumers - the alignment, the depth fusion and the depth hand-over. On the host, through the three
hooks that run the kernels' source (rebvio_hip_test_kf_align_host at max_iter 0, rebvio_hip_test_kf_fuse_host,
rebvio_hip_test_kf_handover_host): for one pose, one filter and a successor as large as the map, a keyframe keyline has an owner in
one of them if and only if it has one in the others, and it is the same owner. The oracle's 160x120 frame with the crafted keyframe
keylines of kf_align_ref.craft_against and one planted keyline per exit of the lookup (kf_align_ref.lookup_case); the restatement
says first that every exit is taken and that at least half of the keylines come through."""
import numpy as np

from kf_align_ref import LOOKUP_EXITS, assert_lookup_case_is_not_vacuous, lookup_case, oracle_scene
from kf_fuse_ref import INT_MIN
from kf_pose_ref import true_motion
from support import F32
from support import backend  # noqa: F401


def assert_same_owners(align, fuse, handover, want):
    """the iff of the module's docstring over three assoc arrays, and `want` = the restatement's mask of associated keylines"""
    a_has, f_has, h_has = align >= 0, fuse != INT_MIN, handover != INT_MIN
    assert np.array_equal(a_has, f_has) and np.array_equal(a_has, h_has), (np.flatnonzero(a_has != f_has)[:8], np.flatnonzero(a_has != h_has)[:8])
    owner = lambda x: np.where(x >= 0, x, -1 - x.astype(np.int64))
    assert np.array_equal(owner(fuse)[a_has], align[a_has]) and np.array_equal(owner(handover)[a_has], align[a_has])
    assert np.array_equal(a_has, want), np.flatnonzero(a_has != want)[:8]


def test_alignment_fusion_and_handover_find_the_same_owners(backend, orc_mod):
    B = backend
    sc = oracle_scene(orc_mod)
    case = lookup_case(sc["cam"], sc["pos"], sc["unit"], sc["ids"], sc["dists"], sc["craft"], room=1 << 20, zero_gradient=True)
    assert set(case["plants"]) == set(LOOKUP_EXITS)
    n = len(case["prs4"])
    want = assert_lookup_case_is_not_vacuous(sc["cam"], case["prs4"], case["normals"], case["pos"], case["unit"], case["ids"], case["dists"],
                                             case["max_dist"], case["plants"], np.ones(n, bool))
    print(f"{n} keyframe keylines, {int(want.sum())} associated, max_dist {case['max_dist']}, plants {case['plants']}")
    R, t = true_motion()
    args = (*sc["cam"], sc["search_range"], case["prs4"], case["kf_matches"], case["normals"], case["pos"], case["unit"], case["ids"],
            case["dists"])
    md = dict(max_dist=case["max_dist"])
    _, align = B.kf_align_host(*args, B.default_kf_align_opts(max_iter=0, **md), R, t)
    _, _, _, fuse = B.kf_fuse_host(*args, B.default_kf_fuse_opts(**md), R, t)
    dst = np.zeros((len(case["pos"]), 4), F32)
    dst[:, 2:] = (1.0, 0.5)
    _, _, _, handover = B.kf_handover_host(*args, dst, np.ones(len(dst), np.uint32), B.default_kf_handover_opts(**md), R, t)
    assert_same_owners(align, fuse, handover, want)
