"""What the tests of rebvio_hip_map_keyframe_align_many share, on top of kf_align_ref.py: the inlier count and the 13 starts restated
in numpy, the ranking restated in Python, and small builders for hypothesis and result arrays. A plain helper module like
kf_align_ref.py: no test lives here and importing it needs no GPU."""
import numpy as np

from kf_align_ref import _residual, cam_of, current_data, np_kf_align_sums  # noqa: F401  (cam_of / current_data: handed on to the device tests)
from kf_pose_ref import DEFAULT_FILTER
from support import F32

ROT_STEP, TRANS_STEP = 0.03, 0.12      # the multi-start steps: the offset the basin table of DESIGN.md 5i still converges from
FAR_OFFSET = (0.05, 0.2)               # the offset that table fails at


def np_inliers(cam, prs4, kf_matches, normals, cur_pos, cur_unit, ids, dists, R, t, flt=DEFAULT_FILTER, huber=2.0, min_cos=0.9, max_dist=40):
    """(inliers, used, guards) of one evaluation at (R, t): the used terms of kf_align_ref.np_kf_align_sums with |e| <= huber; guards
    as there (guards["huber"] = the smallest distance of a used |e| from the switch)"""
    fm, cx, cy, rows, cols = cam
    _, _, used, assoc, g = np_kf_align_sums(cam, prs4, kf_matches, normals, cur_pos, cur_unit, ids, dists, R, t, flt, huber, min_cos, max_dist)
    if not used:
        return 0, 0, g
    pos = np.asarray(cur_pos, F32).reshape(-1, 2)
    unit = np.asarray(cur_unit, F32).reshape(-1, 2)
    q = (pos - np.array([F32(cx), F32(cy)], F32)).astype(F32)
    e = _residual(fm, np.asarray(prs4, F32).reshape(-1, 4), q, unit, np.where(assoc >= 0, assoc, 0), R, t)
    return int((np.abs(e[assoc >= 0]) <= huber).sum()), used, g


def np_exp_left(w, R):
    """E R with the E = (I + A K) + B (K K) of the Gauss-Newton step (include/rebvio_hip.h), first-order below th2 < 1e-16"""
    w = np.asarray(w, np.float64)
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th2 < 1e-16:
        E = np.eye(3) + K
    else:
        th = np.sqrt(th2)
        E = (np.eye(3) + (np.sin(th) / th) * K) + ((1.0 - np.cos(th)) / th2) * (K @ K)
    return E @ np.asarray(R, np.float64).reshape(3, 3)


def np_around(R, t, rot_step, trans_step):
    """the 13 (R, t) of rebvio_hip_kf_hypotheses_around, in its order"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    out = [(R.copy(), t.copy()) for _ in range(13)]
    for a in range(3):
        for s in range(2):
            w = np.zeros(3)
            w[a] = -rot_step if s else rot_step
            out[1 + 2 * a + s] = (np_exp_left(w, R), t.copy())
            tt = t.copy()
            tt[a] = t[a] - trans_step if s else t[a] + trans_step
            out[7 + 2 * a + s] = (R.copy(), tt)
    return out


def py_best(rows, min_inliers):
    """rebvio_hip_kf_align_best on (status, inliers, cost) triples"""
    ok = [(-inl, cost, k) for k, (status, inl, cost) in enumerate(rows) if status == 0 and inl >= min_inliers]
    return min(ok)[2] if ok else -1


def results_of(B, rows):
    """KfHypResult list from (status, inliers, cost) triples; every other field zero"""
    out = []
    for status, inl, cost in rows:
        r = B.KfHypResult()
        r.pose.status, r.inliers, r.pose.cost = status, inl, cost
        out.append(r)
    return out


def hyp_Rt(h):
    return np.array(h.R0).reshape(3, 3), np.array(h.t0)


def seeded_guesses(n, seed, R, t, rot=0.01, trans=0.04):
    """n guesses within rot rad / trans units of (R, t): small seeded rotations (applied on the left) and translations"""
    from support import rodrigues
    rng = np.random.default_rng(seed)
    return [(rodrigues(rng.uniform(-rot, rot, 3)) @ R, t + rng.uniform(-trans, trans, 3)) for _ in range(n)]


# ---- device scenes (the GPU tests; B = the backend module) ------------------------------------------------------------------------
W, H, NF, TS_US = 160, 120, 10, 50000
# every full map holds exactly 800 keylines; gain 0 turns the threshold servo off, so a frame's candidates do not depend on what was
# detected before it
KW_800 = dict(keylines_ref=799, keylines_max=800, global_min_matches_threshold=1, gain=0.0)
_STREAM = {}


def stream():
    if "s" not in _STREAM:
        from rebvio_amd import synth
        _STREAM["s"] = synth.render_stream(W, H, NF)
    return _STREAM["s"]


class Scene800:
    """One context of keylines_max 800 on the 160x120 stream: a detected current map `mc` and snapshots of ANY size 0..800 in that
    one context. A map of exactly n keylines is detected from frame 1 through a static detection mask that lets the first p pixels in
    raster order through: a masked pixel is skipped like one that fails the magnitude test and keylines_max counts the survivors in
    raster order (include/rebvio_hip.h), so with the servo off the size is a non-decreasing function of p with steps of at most 1, and
    p is found by bisection. Crafted keyframe keylines (kf_align_ref.craft_against, against mc) are uploaded into that map and
    snapshotted. snapshot(n) returns (KfSnapshot, restatement data)."""

    def __init__(self, B, seed=1):
        from conftest import params_for
        from kf_align_ref import craft_against, craft_kf_keylines
        frames, cam = stream()
        self.B, self.frame = B, frames[1]
        self.ctx = B.Context(params_for(B, cam, **KW_800))
        self.mc = self.ctx.detect_u8(frames[2], TS_US)
        full = self.ctx.detect_u8(frames[1], 0)
        assert full.size() == 800 == self.mc.size()
        self.kl, self.cur = current_data(self.mc)
        self.A = craft_against(self.kl, self.cur[2], self.cur[3], seed, cam_of(self.ctx))
        base = full.keylines()
        base["matches"] = 0                                     # keylines behind the crafted ones are filtered out
        self.kf = craft_kf_keylines(base, self.A, min(len(self.A["prs4"]), len(base)))
        full.release()
        self.snaps, self.maps = [], []

    def _masked(self, p):
        mask = np.zeros(H * W, np.uint8)
        mask[:p] = 1
        self.ctx.set_detection_mask(mask.reshape(H, W))
        m = self.ctx.detect_u8(self.frame, 0)
        self.ctx.set_detection_mask(None)
        return m

    def sized_map(self, n):
        """a detected map of exactly n keylines"""
        lo, hi = 0, H * W                                       # size(lo) <= n <= size(hi) throughout
        while hi - lo > 1:
            mid = (lo + hi) // 2
            m = self._masked(mid)
            lo, hi = (mid, hi) if m.size() < n else (lo, mid)
            m.release()
        m = self._masked(hi if n else 0)
        assert m.size() == n, (n, m.size())
        self.maps.append(m)
        return m

    def snapshot(self, n, normals=True, dead=False):
        m = self.sized_map(n)
        kf = self.kf[:n].copy()
        if dead:
            kf["matches"] = 0
        m.upload(kf)
        snap = m.keyframe_snapshot()
        if normals:
            snap.add_normals(m)
        prs4, mt = snap.download()
        assert len(prs4) == n
        self.snaps.append(snap)
        return snap, (cam_of(self.ctx), prs4, mt, snap.normals() if normals else None, *self.cur)

    def close(self):
        for s in self.snaps:
            s.release()
        self.ctx.close()
