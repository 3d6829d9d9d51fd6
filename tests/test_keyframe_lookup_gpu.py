"""tests/test_keyframe_lookup.py on the device: rebvio_hip_map_keyframe_align at max_iter 0, rebvio_hip_kf_snapshot_fuse_depth and
rebvio_hip_kf_snapshot_handover_depth (k_kf_align_sums, k_kf_fuse_depth, k_kf_handover_claim - the three kernels kfp::lookup is
inlined into) on one detected 160x120 map, one crafted snapshot, one pose and one filter, the successor being the map's own snapshot:
a keyframe keyline has an owner in one of them if and only if it has one in the others, and it is the same owner. The restatement,
on what was downloaded just before, says first that every planted exit is taken and that at least half of the keylines come through.

Five of the six exits are planted. The sixth, an owner whose gradient has no direction, cannot be: the entries take a detected map
only (an uploaded one is refused with -7) and detection emits no keyline with a zero gradient. The host half covers it."""
import numpy as np
import pytest

from conftest import params_for
from kf_align_many_ref import cam_of, current_data, stream
from kf_align_ref import LOOKUP_EXITS, assert_lookup_case_is_not_vacuous, craft_against, craft_kf_keylines, lookup_case
from kf_fuse_ref import INT_MIN
from kf_pose_ref import DEFAULT_FILTER, true_motion
from support import B  # noqa: F401
from support import TS, np_passes

pytestmark = pytest.mark.gpu


def test_alignment_fusion_and_handover_find_the_same_owners_on_the_device(B):
    frames, cam = stream()
    ctx = B.Context(params_for(B, cam))
    maps = [ctx.detect_u8(frames[k], k * TS) for k in range(3)]
    mk, mc = maps[1], maps[2]
    kl, cur = current_data(mc)
    A = craft_against(kl, cur[2], cur[3], 1, cam_of(ctx))
    case = lookup_case(cam_of(ctx), *cur, A, room=mk.size(), zero_gradient=False)
    assert set(case["plants"]) == set(LOOKUP_EXITS[:5])
    base = mk.keylines()
    base["matches"] = 0                                          # keylines behind the crafted and planted ones are filtered out
    mk.upload(craft_kf_keylines(base, case))
    src = mk.keyframe_snapshot()
    src.add_normals(mk)
    dst = mc.keyframe_snapshot()
    prs4, mt = src.download()
    flt_ok = np_passes(dict(rho=prs4[:, 2], sigma_rho=prs4[:, 3], matches=mt), *DEFAULT_FILTER)
    want = assert_lookup_case_is_not_vacuous(cam_of(ctx), prs4, src.normals(), *cur, case["max_dist"], case["plants"], flt_ok)
    print(f"{len(prs4)} keyframe keylines, {int(want.sum())} associated, max_dist {case['max_dist']}, plants {case['plants']}")
    R, t = true_motion()
    md = dict(max_dist=case["max_dist"])
    _, align = mc.keyframe_align(src, B.default_kf_align_opts(ctx, max_iter=0, **md), R, t, want_assoc=True)
    _, handover = dst.handover_depth(src, mc, R, t, B.default_kf_handover_opts(ctx, **md), want_assoc=True)       # (src is only read)
    _, fuse = src.fuse_depth(mc, R, t, B.default_kf_fuse_opts(ctx, **md), want_assoc=True)
    a_has, f_has, h_has = align >= 0, fuse != INT_MIN, handover != INT_MIN
    assert np.array_equal(a_has, f_has) and np.array_equal(a_has, h_has), (np.flatnonzero(a_has != f_has)[:8], np.flatnonzero(a_has != h_has)[:8])
    owner = lambda x: np.where(x >= 0, x, -1 - x.astype(np.int64))
    assert np.array_equal(owner(fuse)[a_has], align[a_has]) and np.array_equal(owner(handover)[a_has], align[a_has])
    assert np.array_equal(a_has, want), np.flatnonzero(a_has != want)[:8]
    src.release()
    dst.release()
    ctx.close()
