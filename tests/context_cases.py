"""Contexts away from the default one, stated once, for the entries that go through kfp::lookup (rebvio_amd/csrc/kf_pose.hpp): the
keyframe alignment, the many-hypothesis alignment, the snapshot depth fusion and the depth hand-over. The lookup is the one place
outside detection that reads a context's geometry - fm, the principal point, rows / cols, df_nr = 2 * search_range in the decode of
the device's field key, the cap - and every other test of those entries builds its camera with synth.Camera.for_size (cx = W / 2,
cy = H / 2) and keeps search_range at 40. The rows here move each of them; tests/test_context_geometry.py runs them through the host
hooks and tests/test_context_geometry_gpu.py on the device. A plain helper module like place_cases.py and stereo_prior_cases.py: no
test lives here and importing it needs no GPU."""
import numpy as np

from kf_align_ref import (_lookup, assert_lookup_case_is_not_vacuous, cam_of, craft_against, craft_kf_keylines, current_data, data_of,
                          lookup_case, oracle_scene)
from kf_pose_ref import DEFAULT_FILTER, true_motion
from support import F32, TS, np_passes

# id: frame, camera, search_range, other parameters - and what the row is for
CONTEXTS = {
    # an odd, ragged width (no multiple of a wave, a tile or 4), a quarter-pixel principal point off the centre, df_nr 14
    "A": dict(width=131, height=67, fm=97.3, cx=71.25, cy=29.5, search_range=7.0, other={}),
    # EuRoC's intrinsics over four, df_nr 6
    "B": dict(width=188, height=120, fm=114.49, cx=91.8, cy=62.1, search_range=3.0, other={}),
    # the principal point near a corner, a half-integer cx, a long focal length, distances past 40
    "C": dict(width=160, height=120, fm=300.0, cx=20.5, cy=100.25, search_range=100.0, other=dict(pixel_uncertainty_match=1.0)),
    # df_nr 510: distances that need bits 7 and 8 of the key's distance field (the camera is the synthetic one)
    "D": dict(width=160, height=120, fm=114.5, cx=80.0, cy=60.0, search_range=255.0, other=dict(pixel_uncertainty_match=1.0)),
}
IDS = tuple(CONTEXTS)
# KW_FULL of the alignment tests; keylines_max * df_nr stays below 2^23 in D (1601 * 510)
KW_KEYLINES = dict(keylines_ref=1200, keylines_max=1601, global_min_matches_threshold=1)
SIDES = ("x = 0", "x = cols - 1", "y = 0", "y = rows - 1")
# the sides of the frame a row's scene has to carry a rim plant on (context_cases.rim_plants): "x = cols - 1" and "y = rows - 1" are
# the ones the border test's cols - 2 and rows - 2 decide. With search_range 3 (B) few keylines reach the rim: the bottom row has none.
HOST_SIDES = dict(A=SIDES, B=SIDES[:3], C=SIDES, D=SIDES)
DEVICE_SIDES = dict(A=SIDES, B=SIDES[:3], C=SIDES, D=SIDES)
NF = 3      # frames of the synthetic stream a scene uses: the keyframe is detected on frame 1, the current map on frame 2


def context_kw(cid, **over):
    """the parameters of row `cid` as keyword arguments of default_params; fm, cx and cy as the fp32 values a context holds"""
    c = CONTEXTS[cid]
    kw = dict(fm=float(F32(c["fm"])), cx=float(F32(c["cx"])), cy=float(F32(c["cy"])), search_range=c["search_range"], **KW_KEYLINES, **c["other"])
    kw.update(over)
    return kw


def context_params(mod, cid, **over):
    """default_params of `mod` (the backend or the oracle) for row `cid`"""
    c = CONTEXTS[cid]
    return mod.default_params(c["height"], c["width"], **context_kw(cid, **over))


_FRAMES = {}


def frames_of(cid):
    """the NF frames of the synthetic stream at the row's size (rendered for the synthetic camera: an image is an image)"""
    c = CONTEXTS[cid]
    key = (c["width"], c["height"])
    if key not in _FRAMES:
        from rebvio_amd import synth
        _FRAMES[key] = synth.render_stream(c["width"], c["height"], NF)[0]
    return _FRAMES[key]


# ---- planted keyframe keylines -----------------------------------------------------------------------------------------------------
def onto(cam, x, y, normal):
    """the keyframe keyline that the crafted motion projects 0.2 px off the centre of cell (x, y), made as kf_align_ref.lookup_case
    makes its plants - the point of that pixel at depth 1, taken back through the motion: (prs4 row, normal)"""
    fm, cx, cy, rows, cols = cam
    R, t = true_motion()
    ray = np.array([(x + 0.2 - np.float64(F32(cx))) / np.float64(F32(fm)), (y - 0.2 - np.float64(F32(cy))) / np.float64(F32(fm)), 1.0])
    X = R.T @ (ray - t)
    n = R[:2, :2].T @ np.asarray(normal, np.float64)
    return [fm * X[0] / X[2], fm * X[1] / X[2], 1.0 / X[2], 0.05 / X[2]], n / np.linalg.norm(n)


def with_plants(case, rows4, normals, names):
    """`case` (a dict with prs4, kf_matches, normals and more) with planted keylines behind it; returns (new dict, {name: index})"""
    n = len(case["prs4"])
    out = dict(case)
    out["prs4"] = np.concatenate([case["prs4"], np.array(rows4, F32).reshape(-1, 4)]).astype(F32)
    out["kf_matches"] = np.concatenate([case["kf_matches"], np.full(len(rows4), 3, np.uint32)])
    out["normals"] = np.concatenate([case["normals"], np.array(normals, F32).reshape(-1, 2)]).astype(F32)
    return out, {name: n + k for k, name in enumerate(names)}


def rim_plants(cam, unit, ids, dists, max_dist):
    """Per side of the frame: a keyline that lands in a cell of the outermost column / row which a keyline owns within max_dist with
    a gradient - nothing but the border test against 1 and cols - 2 / rows - 2 keeps it out - and a control in the column / row
    next to it, likewise owned, which is associated. Their normals are the owners' units, so the gradient test lets them through. A
    side with no such pair of cells is left out. Returns (prs4 rows, normals, names): names "x = 0", "x = 1", "x = cols - 1",
    "x = cols - 2", "y = 0", ... in pairs, the outer one first."""
    fm, cx, cy, rows, cols = cam
    ids2, dists2 = np.asarray(ids).reshape(rows, cols), np.asarray(dists).reshape(rows, cols)
    unit = np.asarray(unit, F32).reshape(-1, 2)
    has_dir = np.zeros((rows, cols), bool)
    has_dir[ids2 >= 0] = (unit[ids2[ids2 >= 0]].astype(np.float64) ** 2).sum(1) > 0
    ok = (ids2 >= 0) & (dists2 <= max_dist) & has_dir
    rows4, normals, names = [], [], []
    for outer, inner in (("x = 0", "x = 1"), ("x = cols - 1", "x = cols - 2"), ("y = 0", "y = 1"), ("y = rows - 1", "y = rows - 2")):
        along_x = outer[0] == "y"
        fixed = {"x = 0": 0, "x = 1": 1, "x = cols - 1": cols - 1, "x = cols - 2": cols - 2, "y = 0": 0, "y = 1": 1, "y = rows - 1": rows - 1,
                 "y = rows - 2": rows - 2}
        cell = lambda name, k: (k, fixed[name]) if along_x else (fixed[name], k)      # (x, y)
        span = range(2, (cols if along_x else rows) - 2)
        found = {name: next((k for k in span if ok[cell(name, k)[1], cell(name, k)[0]]), None) for name in (outer, inner)}
        if None in found.values():
            continue
        for name in (outer, inner):
            x, y = cell(name, found[name])
            row, nrm = onto(cam, x, y, unit[ids2[y, x]].astype(np.float64))
            rows4.append(row)
            normals.append(nrm)
            names.append(name)
    return rows4, normals, names


def full_case(cam, pos, unit, ids, dists, A, room, zero_gradient):
    """kf_align_ref.lookup_case with the rim plants behind its own: (case, {side or control: keyframe keyline})"""
    case = lookup_case(cam, pos, unit, ids, dists, A, room=room - 2 * len(SIDES), zero_gradient=zero_gradient)
    rows4, normals, names = rim_plants(cam, case["unit"], ids, dists, case["max_dist"])
    return with_plants(case, rows4, normals, names)


def distance_case(cam, kl, cur, room, seed=1, displaced=0.2, first=2):
    """Keyframe keylines whose lookups land away from their owners, for the sweep of max_dist with the gradient gate off: the crafted
    keylines of craft_against with a share of them displaced by 15 px along their normal, and behind them one planted keyline per
    distance d >= first that a cell inside the border has in the field - landing in the first such cell in raster order. `room`
    keylines at the most; the plants are kept, the crafted ones cut. Returns dict(prs4, kf_matches, normals, plant_dist int [n]:
    the distance of a plant's cell, -1 for a crafted keyline)."""
    fm, cx, cy, rows, cols = cam
    pos, unit, ids, dists = cur
    ids2, dists2 = np.asarray(ids).reshape(rows, cols), np.asarray(dists).reshape(rows, cols)
    inner = np.zeros((rows, cols), bool)
    inner[1:rows - 1, 1:cols - 1] = True
    owned = (ids2 >= 0) & inner
    rows4, normals, plant_d = [], [], []
    for d in np.unique(dists2[owned]):
        if d < first:
            continue
        y, x = np.argwhere(owned & (dists2 == d))[0]
        row, nrm = onto(cam, x, y, np.asarray(unit, F32).reshape(-1, 2)[ids2[y, x]].astype(np.float64))
        rows4.append(row)
        normals.append(nrm)
        plant_d.append(int(d))
    A = craft_against(kl, ids, dists, seed, cam, displaced)
    n = min(len(A["prs4"]), room - len(rows4))
    assert n > 0
    case, _ = with_plants(dict(prs4=A["prs4"][:n], kf_matches=A["kf_matches"][:n], normals=A["normals"][:n]), rows4, normals, plant_d)
    case["plant_dist"] = np.concatenate([np.full(n, -1), np.array(plant_d, np.int64)]).astype(np.int64)
    return case


def successor_records(prop, m, seed, base):
    """rho, sigma_rho and matches for a successor of m slots, as tests/test_keyframe_handover_gpu.py builds it: slot i carries what
    the outgoing keyframe propagates to it (prop: np_kf_handover into a blank successor), moved by a seeded draw of 10 %, with
    sigma_rho between 0.01 and 0.3 of rho - so slots are adopted, kept and in conflict - and rho 1, sigma_rho 0.5 where nothing
    lands. Written into a copy of the keyline array `base` [m]."""
    rng = np.random.default_rng(seed)
    kl = base.copy()
    rho, sig = np.ones(m), np.full(m, 0.5)
    win = prop["winner"][:m]
    has = win >= 0
    rho[has] = prop["rho_c"][win[has]] * (1.0 + 0.1 * np.clip(rng.standard_normal(int(has.sum())), -2.5, 2.5))
    sig[has] = rho[has] * rng.choice([0.01, 0.04, 0.1, 0.3], int(has.sum()))
    kl["rho"], kl["sigma_rho"], kl["matches"] = rho.astype(F32), sig.astype(F32), rng.integers(0, 6, m).astype(np.uint32)
    return kl


def assert_rim_plants(cam, prs4, normals, pos, unit, ids, dists, max_dist, plants, need):
    """on the restatement, at the crafted motion and min_cos 0.9: every side of `need` is planted; an outer plant leaves at the border
    test while the cell it lands in is owned within max_dist, and its control next to it is associated"""
    fm, cx, cy, rows, cols = cam
    planted = [s for s in SIDES if s in plants]
    assert set(need) <= set(planted), (need, planted)
    R, t = true_motion()
    ok, i, g = _lookup(cam, prs4, normals, pos, unit, ids, dists, R, t, 0.9, max_dist)
    # the same lookup on the same field with two empty cells around it and the principal point moved along: the border is elsewhere
    wide = (fm, float(F32(cx) + F32(2)), float(F32(cy) + F32(2)), rows + 4, cols + 4)
    pad = lambda a, fill: np.pad(np.asarray(a).reshape(rows, cols), 2, constant_values=fill).reshape(-1)
    okw, iw, _ = _lookup(wide, prs4, normals, pos, unit, pad(ids, -1), pad(dists, 0x7FFFFFFF), R, t, 0.9, max_dist)
    inner = {"x = 0": "x = 1", "x = cols - 1": "x = cols - 2", "y = 0": "y = 1", "y = rows - 1": "y = rows - 2"}
    for s in planted:
        j, jc = plants[s], plants[inner[s]]
        assert not ok[j] and g["why"][j] == 2, (s, int(g["why"][j]))
        assert okw[j], s                                         # nothing but the border test keeps the outer plant out
        assert ok[jc] and okw[jc] and i[jc] == iw[jc], (inner[s], int(g["why"][jc]))
    return planted


# ---- the host half: the oracle's frame -------------------------------------------------------------------------------------------
def host_scene(O, cid):
    """kf_align_ref.oracle_scene for row `cid`: frame 2 of the stream at the row's size, detected by an oracle of the row's
    parameters, with the row's camera in scene["cam"]. Computed once per row; read-only."""
    c = CONTEXTS[cid]
    sc = oracle_scene(O, frame=NF - 1, width=c["width"], height=c["height"], **context_kw(cid))
    assert sc["cam"] == (float(F32(c["fm"])), float(F32(c["cx"])), float(F32(c["cy"])), c["height"], c["width"])
    assert sc["search_range"] == int(c["search_range"])
    return sc


def host_case(O, cid):
    """(scene, lookup case with all six exits planted, restatement's mask of associated keylines): the non-vacuity of the row is
    asserted here, on the restatement, before a caller compares anything"""
    sc = host_scene(O, cid)
    case, rim = full_case(sc["cam"], sc["pos"], sc["unit"], sc["ids"], sc["dists"], sc["craft"], room=1 << 20, zero_gradient=True)
    args = (sc["cam"], case["prs4"], case["normals"], case["pos"], case["unit"], case["ids"], case["dists"], case["max_dist"])
    want = assert_lookup_case_is_not_vacuous(*args, case["plants"], np.ones(len(case["prs4"]), bool))
    case["rim"] = rim
    case["sides"] = assert_rim_plants(*args, rim, need=HOST_SIDES[cid])
    return sc, case, want


# ---- the device half: a map the device detected ------------------------------------------------------------------------------------
class DeviceScene:
    """One context of row `cid` with two detected maps - the keyframe's `mk` (frame 1) and the current `mc` (frame 2) - and what the
    restatement is given of mc: `kl`, `cur` = (pos, unit, ids, dists), downloaded once. mc is never uploaded to (the entries refuse
    a map whose field is not detection's); mk takes crafted keyframe keylines by upload, snapshot after snapshot."""

    def __init__(self, B, cid, **over):
        self.B, self.cid = B, cid
        frames = frames_of(cid)
        self.ctx = B.Context(context_params(B, cid, **over))
        self.mk, self.mc = [self.ctx.detect_u8(frames[1 + k], k * TS) for k in range(2)]
        self.kl, self.cur = current_data(self.mc)
        self.cam = cam_of(self.ctx)
        self.base = self.mk.keylines()
        self.base["matches"] = 0                                 # keylines behind the crafted and planted ones are filtered out
        self.snaps = []

    def snapshot(self, kf_keylines, normals=True, n=None):
        """the keyframe keylines uploaded into mk (cut at n) and snapshotted: (KfSnapshot, restatement data)"""
        self.mk.upload(kf_keylines)
        snap = self.mk.keyframe_snapshot()
        if normals:
            snap.add_normals(self.mk)
        self.snaps.append(snap)
        return snap, data_of(self.ctx, snap, self.cur, normals)

    def crafted(self, seed=1, displaced=0.0):
        """crafted_scene of the alignment tests: (snapshot, restatement data, crafted arrays)"""
        A = craft_against(self.kl, self.cur[2], self.cur[3], seed, self.cam, displaced)
        snap, D = self.snapshot(craft_kf_keylines(self.base, A, min(len(A["prs4"]), len(self.base))))
        return snap, D, A

    def planted(self, seed=1):
        """the crafted keylines with the five exits a detected map can carry planted behind them: (snapshot, restatement data, case,
        restatement's mask of associated keylines) - non-vacuity asserted on the snapshot's download"""
        A = craft_against(self.kl, self.cur[2], self.cur[3], seed, self.cam)
        case, rim = full_case(self.cam, *self.cur, A, room=len(self.base), zero_gradient=False)
        snap, D = self.snapshot(craft_kf_keylines(self.base, case))
        prs4, mt = D[1], D[2]
        flt_ok = np_passes(dict(rho=prs4[:, 2], sigma_rho=prs4[:, 3], matches=mt), *DEFAULT_FILTER)
        want = assert_lookup_case_is_not_vacuous(self.cam, prs4, D[3], *self.cur, case["max_dist"], case["plants"], flt_ok)
        case["rim"] = rim
        case["sides"] = assert_rim_plants(self.cam, prs4, D[3], *self.cur, case["max_dist"], rim, need=DEVICE_SIDES[self.cid])
        return snap, D, case, want

    def close(self):
        for s in self.snaps:
            s.release()
        self.ctx.close()
