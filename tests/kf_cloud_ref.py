"""The point cloud of a keyframe snapshot (rebvio_hip_kf_snapshot_point_cloud) as the existing reference model sees it:
support.np_cloud - the numpy fp32 restatement of a map's cloud, checked by hand in tests/test_point_cloud.py - applied to a
structured array made of a snapshot's download, with gradient_norm 0 and the index as the keyline. Plus the seeded snapshots the
CPU and GPU tests share. A plain helper module like support.py and kf_fuse_ref.py: no test lives here and importing it needs no GPU."""
import numpy as np

from support import CLOUD_DTYPE, F32, np_cloud

SNAP_DTYPE = np.dtype([("pos_img", "<f4", (2,)), ("rho", "<f4"), ("sigma_rho", "<f4"), ("gradient_norm", "<f4"), ("matches", "<u4")])
DEFAULT = (2, F32(0.5), F32(1e-3), F32(20.0))        # rebvio_hip_default_cloud_filter
ODD = (3, F32(0.3), F32(0.1), F32(4.0))              # a filter every term of which cuts into random_snapshot's draws
SIZES = (0, 1, 63, 64, 65, 255, 256, 257)            # wave and workgroup edges
UP, DOWN = F32(np.inf), F32(-np.inf)


def snapshot_keylines(prs4, matches):
    """(prs4 float32 [n, 4], matches uint32 [n]) of KfSnapshot.download as the records np_cloud reads"""
    prs4 = np.asarray(prs4, F32).reshape(-1, 4)
    kl = np.zeros(len(prs4), SNAP_DTYPE)
    kl["pos_img"], kl["rho"], kl["sigma_rho"], kl["matches"] = prs4[:, :2], prs4[:, 2], prs4[:, 3], np.asarray(matches, np.uint32)
    return kl


def np_kf_cloud(prs4, matches, fm, flt=DEFAULT, pose=None):
    c = np_cloud(snapshot_keylines(prs4, matches), fm, flt, pose)
    assert c.dtype == CLOUD_DTYPE and not c["gradient_norm"].view(np.uint32).any()       # +0.0f, every bit
    return c


def flt_dict(flt):
    return dict(min_matches=int(flt[0]), max_rel_sigma=float(flt[1]), rho_min=float(flt[2]), rho_max=float(flt[3]))


def edge_rows(flt):
    """Every filter term exactly on its bound and one ulp (one count) outside it, and the values no positive test lets through:
    rows of (pos_img x, y, rho, sigma_rho, matches, passes)"""
    mm, rel, lo, hi = int(flt[0]), F32(flt[1]), F32(flt[2]), F32(flt[3])
    rho = F32(0.7)
    bound = F32(rel * rho)                                   # one rounded fp32 multiply
    mid = F32(0.5) * (lo + hi)
    ok_sig = F32(0.0)
    rows = [(3.0, -2.0, mid, ok_sig, mm, True), (3.0, -2.0, mid, ok_sig, mm - 1, False),
            (-7.5, 4.0, lo, ok_sig, mm, True), (-7.5, 4.0, np.nextafter(lo, DOWN), ok_sig, mm, False),
            (11.0, 9.0, hi, ok_sig, mm, True), (11.0, 9.0, np.nextafter(hi, UP), ok_sig, mm, False),
            (-1.0, -1.0, rho, bound, mm, True), (-1.0, -1.0, rho, np.nextafter(bound, UP), mm, False),
            (2.0, 2.0, np.nan, ok_sig, mm, False), (2.0, 2.0, np.inf, ok_sig, mm, False), (2.0, 2.0, 0.0, ok_sig, mm, False),
            (2.0, 2.0, -1.0, -1.0, mm, False), (2.0, 2.0, rho, np.nan, mm, False), (2.0, 2.0, rho, np.inf, mm, False),
            (2.0, 2.0, np.nan, np.nan, mm, False), (2.0, 2.0, rho, -0.5, 0xFFFFFFFF, True)]
    return [(F32(x), F32(y), F32(r), F32(s), np.uint32(m & 0xFFFFFFFF), p) for x, y, r, s, m, p in rows if m >= 0]


def random_snapshot(n, seed, flt=DEFAULT, plant=True):
    """(prs4, matches) of n seeded records: matches 0..5, rho over the filter's range and a little beyond, sigma_rho up to 1.5 x the
    filter's bound; with plant, the rows of edge_rows(flt) at seeded places (as many as fit)."""
    rng = np.random.default_rng(seed)
    prs4 = np.zeros((n, 4), F32)
    prs4[:, :2] = rng.uniform(-80.0, 80.0, (n, 2))
    prs4[:, 2] = np.exp(rng.uniform(np.log(0.5 * float(flt[2])), np.log(1.5 * float(flt[3])), n))
    prs4[:, 3] = prs4[:, 2] * (rng.uniform(0.0, 1.5 * float(flt[1]), n)).astype(F32)
    mt = rng.integers(0, 6, n).astype(np.uint32)
    if plant and n:
        rows = edge_rows(flt)
        at = rng.permutation(n)[:len(rows)]
        for i, (x, y, r, s, m, _) in zip(at, rows):
            prs4[i] = (x, y, r, s)
            mt[i] = m
    return prs4, mt


def random_pose(seed):
    """a rotation of 1.1 rad about a seeded axis, a seeded shift, scale 0.37 (the pose of tests/test_point_cloud_gpu.py)"""
    rng = np.random.default_rng(seed)
    w = rng.normal(size=3)
    w *= 1.1 / np.linalg.norm(w)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    return R.astype(F32), rng.normal(size=3).astype(F32), F32(0.37)


def assert_cloud_equal(got, want, what):
    assert got.dtype == CLOUD_DTYPE, got.dtype
    assert len(got) == len(want), f"{what}: {len(got)} points, expected {len(want)}"
    for f in CLOUD_DTYPE.names if len(got) else ():
        a, b = np.ascontiguousarray(got[f]).view(np.uint32), np.ascontiguousarray(want[f]).view(np.uint32)
        bad = np.flatnonzero((a != b).reshape(len(got), -1).any(axis=1))
        assert bad.size == 0, f"{what}: field {f} differs at {bad.size} points, first {bad[0]}: {got[f][bad[0]]} != {want[f][bad[0]]}"
    assert got.tobytes() == want.tobytes(), what
