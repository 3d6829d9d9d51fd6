"""The depth hand-over between keyframe snapshots on the device: rebvio_hip_kf_snapshot_handover_depth (k_kf_handover_claim,
k_kf_handover_apply). The contracts:
  - every output word - the successor's records and matches, assoc, the seven counts - equals the host hook's
    (rebvio_hip_test_kf_handover_host) and the numpy restatement's (tests/kf_handover_ref.py) on the snapshots, keylines and distance
    field downloaded just before: per-keyline IEEE fp64 in the same order on all sides, integer claims, no sum whose order could
    differ, so equality is the bound. Wave and workgroup edges, collisions of 2, 64 and 257 claimants on one owner, and 65 536
    keylines for the grid at its cap;
  - two runs are equal in every byte, and a second hand-over works on what the first left;
  - every outcome of the definition planted on a detected map is what comes out for exactly that keyline; src is never written;
  - an empty src changes nothing; launches, resources and refusals are as include/rebvio_hip.h documents;
  - nothing of tracking is disturbed.
A comparison is valid only while nothing in the restatement comes within GUARD of a decision; every comparison asserts that first.
Snapshots are crafted (tests/kf_align_many_ref.py: Scene800) on the 160x120 stream with keylines_max 800, all in ONE context, unless
a case says otherwise."""
import ctypes as C

import numpy as np
import pytest

from conftest import params_for
from kf_align_many_ref import Scene800, cam_of, current_data, stream
from kf_align_ref import GUARD, craft_against, craft_kf_keylines
from kf_fuse_ref import INT_MIN
from kf_handover_ref import assert_identities, counts_of, guard_min, np_kf_handover
from kf_pose_ref import true_motion
from support import B, refusal_scene  # noqa: F401
from support import DEAD_MAP, DEAD_SNAPSHOT, assert_refused, foreign_snapshot, no_field
from support import F32, TS, enlarged_stream, rec, same_records

pytestmark = pytest.mark.gpu

W, H = 160, 120
SIZES = (1, 63, 64, 65, 255, 256, 257, 800)
KW_STREAM = dict(keylines_ref=600, keylines_max=800, global_min_matches_threshold=50)      # the stream of the pose tests: every pair tracks
WIDE = dict(min_matches=1, max_rel_sigma=1e9, rho_min=1e-3, rho_max=20.0)


@pytest.fixture(scope="module")
def scene(B):
    """the scene and one outgoing snapshot per size of SIZES (with normals), shared by the tests below and left unchanged by them -
    the entry never writes src"""
    S = Scene800(B)
    S.by_size = {n: S.snapshot(n) for n in SIZES}
    R, t = true_motion()
    full = S.by_size[800][1]
    # what every crafted keyline propagates to, and where: the successors below are built around it
    blank = np.zeros((800, 4), F32)
    blank[:, 2:] = (1.0, 1e9)
    S.prop = np_kf_handover(*full, blank, np.zeros(800, np.uint32), R, t)
    yield S
    S.close()


def np_opts(kw):
    o = dict(kw)
    if "kf_filter" in o:
        f = o.pop("kf_filter")
        o["flt"] = tuple(f[k] for k in ("min_matches", "max_rel_sigma", "rho_min", "rho_max"))
    return o


def successor(S, seed, size=800, rows=None):
    """a dst snapshot of `size` slots in S's context: slot i carries what the crafted keylines propagate to it (S.prop), moved by a
    seeded draw of 10 %, with sigma_rho between 0.01 and 0.3 of rho - so slots are adopted, kept and in conflict - and rho 1,
    sigma_rho 0.5 where nothing lands. rows: {slot: (rho, sigma_rho, matches)} to plant. The records go into a detected map of that
    size by upload (the hand-over reads dst's buffers only; the map it was cut from plays no part)."""
    rng = np.random.default_rng(seed)
    m = S.sized_map(size)
    kl = m.keylines()
    rho = np.ones(size)
    sig = np.full(size, 0.5)
    win = S.prop["winner"][:size]
    has = win >= 0
    rho[has] = S.prop["rho_c"][win[has]] * (1.0 + 0.1 * np.clip(rng.standard_normal(int(has.sum())), -2.5, 2.5))
    sig[has] = rho[has] * rng.choice([0.01, 0.04, 0.1, 0.3], int(has.sum()))
    kl["rho"], kl["sigma_rho"], kl["matches"] = rho.astype(F32), sig.astype(F32), rng.integers(0, 6, size).astype(np.uint32)
    for i, (r, s, mt) in (rows or {}).items():
        kl["rho"][i], kl["sigma_rho"][i], kl["matches"][i] = r, s, mt
    m.upload(kl)
    snap = m.keyframe_snapshot()
    S.snaps.append(snap)
    return snap


def assert_handover(B, S, dst, src, D, R, t, what, mc=None, ctx=None, cur=None, **kw):
    """one hand-over on the device against the restatement and the hook run on D (src's restatement data) and dst's download from
    just before: the guards, then every output word; src byte-identical afterwards. Returns the restatement."""
    ctx, mc = ctx or S.ctx, mc or S.mc
    dp, dm = dst.download()
    args = (*D[:8], dp, dm) if cur is None else (*D[:4], *cur, dp, dm)
    ref = np_kf_handover(*args, R, t, **np_opts(kw))
    assert guard_min(ref) > GUARD, (what, ref["guards"])
    opts = B.default_kf_handover_opts(ctx, **kw)
    hk, hp, hm, ha = B.kf_handover_host(*args[0], int(ctx.p.search_range), *args[1:], opts, R, t)
    got, assoc = dst.handover_depth(src, mc, R, t, opts, want_assoc=True)
    prs4, mt = dst.download()
    for side, (cn, p, m, a) in (("hook", (hk, hp, hm, ha)), ("device", (got, prs4, mt, assoc))):
        assert counts_of(cn) == counts_of(ref), (what, side, counts_of(cn), counts_of(ref))
        assert np.array_equal(a, ref["assoc"]), (what, side, np.flatnonzero(a != ref["assoc"])[:8])
        assert p.tobytes() == ref["prs4"].tobytes(), (what, side, np.flatnonzero((p != ref["prs4"]).any(1))[:8])
        assert np.array_equal(m, ref["matches"]), (what, side)
    assert_identities(counts_of(got))
    assert got.candidates == len(D[1])
    sp, sm = src.download()
    assert sp.tobytes() == D[1].tobytes() and sm.tobytes() == D[2].tobytes(), what          # src is never written
    assert np.array_equal(prs4[:, :2], dp[:, :2])                                           # nor dst's pos_img
    return ref


# ---- 1. device == hook == restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_handover_from_crafted_snapshots_bit_for_bit(B, scene, n):
    """the wave edge, the workgroup edge and several workgroups as src against an 800-keyline dst; a second hand-over into the same
    dst with other options follows the restatement applied twice: the state is carried across calls"""
    S = scene
    src, D = S.by_size[n]
    dst = successor(S, 100 + n)
    R, t = true_motion()
    first = assert_handover(B, S, dst, src, D, R, t, f"n {n}: first")
    assert n < 63 or (first["associated"] >= 0.7 * n and first["adopted"] > 0.2 * n), counts_of(first)
    assert n < 255 or (first["kept"] > 0 and first["conflicts"] > 0), counts_of(first)
    second = assert_handover(B, S, dst, src, D, R, t, f"n {n}: second", gate_sigma=30.0, q_abs=0.001, max_dist=6, min_cos=-1.0)
    # what the first call adopted is kept now (q_abs makes every propagated sigma larger than the one adopted), and the wider gate
    # turns the former conflicts - slots with a small sigma of their own - into kept ones
    assert second["kept"] >= first["adopted"] and (n < 255 or second["conflicts"] < first["conflicts"]), counts_of(second)
    print(n, counts_of(first), counts_of(second))


def _collide(S, B, n, equal):
    """n src keylines that all land on one owner: copies of one crafted keyline with sigma_rho spread (or all equal)"""
    k0 = int(np.flatnonzero(S.prop["assoc"] != INT_MIN)[0])
    kf = S.kf[:n].copy()
    for f in ("pos_img", "rho", "gradient", "gradient_norm", "matches"):
        kf[f][:] = S.kf[f][k0]
    base = np.float64(S.kf["sigma_rho"][k0])
    mult = np.ones(n) if equal else 1.0 + ((np.arange(n) * 37 + 11) % n) / n
    kf["sigma_rho"] = (base * mult).astype(F32)
    kf["matches"] = (3 + np.arange(n) % 5).astype(np.uint32)
    m = S.sized_map(n)
    m.upload(kf)
    snap = m.keyframe_snapshot()
    snap.add_normals(m)
    S.snaps.append(snap)
    prs4, mt = snap.download()
    owner = -1 - int(S.prop["assoc"][k0]) if S.prop["assoc"][k0] < 0 else int(S.prop["assoc"][k0])
    return snap, (cam_of(S.ctx), prs4, mt, snap.normals(), *S.cur), owner, int(np.argmin(mult))


@pytest.mark.parametrize("n,equal", [(2, False), (64, False), (257, False), (257, True)])
def test_collisions_on_one_owner(B, scene, n, equal):
    """2 claimants, a whole wave, across workgroups - the smallest propagated sigma wins - and 257 with equal sigmas: index 0 wins"""
    S = scene
    src, D, owner, jmin = _collide(S, B, n, equal)
    dst = successor(S, 7, rows={owner: (float(S.prop["rho_c"][S.prop["winner"][owner]]) * 1.01, 0.5, 1)})
    ref = assert_handover(B, S, dst, src, D, *true_motion(), f"collision {n} equal {equal}")
    assert counts_of(ref) == (n, n, 0, 1, 1, 0, 0), counts_of(ref)
    assert ref["winner"][owner] == (0 if equal else jmin)
    assert (ref["assoc"] == owner).sum() == 1 and (ref["assoc"] == -1 - owner).sum() == n - 1
    assert ref["matches"][owner] == max(1, int(D[2][ref["winner"][owner]]))


def test_every_outcome_planted_on_a_detected_map(B, scene):
    """Planted src keylines at R = I, t = (0, 0, tz): Y.z = 1 + rho tz, and a keyline of depth rho with pos_img = (target - (cx, cy)) Y.z
    projects onto the target pixel - the pos of an owner that sits within 0.15 px of its cell's centre. One owner per plant."""
    S = scene
    ctx, mc = S.ctx, S.mc
    pos, unit, ids = S.cur[0], S.cur[1], S.cur[2].reshape(H, W)
    fm, cx, cy = ctx.p.fm, ctx.p.cx, ctx.p.cy

    def good(i):
        x, y = int(round(pos[i, 0])), int(round(pos[i, 1]))
        return 2 <= x <= W - 3 and 2 <= y <= H - 3 and ids[y, x] == i and np.abs(pos[i] - np.round(pos[i])).max() < 0.15 and (unit[i] ** 2).sum() > 0
    own = [i for i in range(800) if good(i)]
    assert len(own) >= 12
    last = max(own)
    #         name             tz      rho     sigma   matches  dst slot (rho, sigma, matches)   outcome
    plants = [("adopted",      -0.02,  1.0,    0.05,   7,       (1.03, 0.2, 2),                 "adopted"),
              ("adopted, max", -0.02,  1.0,    0.05,   7,       (1.03, 0.2, 9),                 "adopted"),
              ("kept",         -0.02,  1.0,    0.05,   7,       (1.03, 0.001, 2),               "kept"),
              ("equal sigma",  -0.02,  1.0,    0.05,   7,       (1.03, None, 2),                "kept"),
              ("conflict",     -0.02,  1.0,    0.05,   7,       (3.0, 0.01, 2),                 "conflict"),
              ("NaN sigma",    -0.02,  1.0,    0.05,   7,       (1.03, np.nan, 2),              "conflict"),
              ("NaN rho",      -0.02,  1.0,    0.05,   7,       (np.nan, 0.2, 2),               "conflict"),
              ("high",         -0.02,  19.5,   0.05,   7,       (1.0, 0.2, 2),                  "range"),
              ("low",          +0.5,   1e-3,   1e-4,   7,       (1.0, 0.2, 2),                  "range"),
              ("filtered",     -0.02,  1.0,    0.05,   0,       (1.03, 0.2, 2),                 "none"),
              ("NaN src sigma", -0.02, 1.0,    np.nan, 7,       (1.03, 0.2, 2),                 "none")]
    P = len(plants)
    owners = own[:P - 1] + [last]
    for tz in (-0.02, +0.5):
        t = np.array([0.0, 0.0, tz])
        kf = S.kf.copy()
        kf["matches"] = 0
        rows = {}
        for k, (name, ptz, rho, sig, mt, (dr, ds, dm), outcome) in enumerate(plants):
            yz = 1.0 + np.float64(F32(rho)) * tz
            kf["pos_img"][k] = (F32((pos[owners[k], 0] - cx) * yz), F32((pos[owners[k], 1] - cy) * yz))
            kf["rho"][k], kf["sigma_rho"][k], kf["matches"][k] = rho, sig, mt if ptz == tz else 0
            kf["gradient"][k] = (F32(10 * unit[owners[k], 0]), F32(10 * unit[owners[k], 1]))
            kf["gradient_norm"][k] = 10.0
            if ds is None:      # the very fp32 the kernel will propagate
                ds = float(F32(abs(1.0 / (yz * yz)) * np.sqrt(np.float64(F32(sig)) ** 2)))
            rows[owners[k]] = (dr, ds, dm)
        m = S.sized_map(800)
        m.upload(kf)
        src = m.keyframe_snapshot()
        src.add_normals(m)
        S.snaps.append(src)
        D = (cam_of(ctx), *src.download(), src.normals(), *S.cur)
        dst = successor(S, 3, rows=rows)
        before = dst.download()
        ref = assert_handover(B, S, dst, src, D, np.eye(3), t, f"plants tz {tz}", kf_filter=WIDE)
        want = {"adopted": lambda i: i, "kept": lambda i: -1 - i, "conflict": lambda i: -1 - i, "range": lambda i: -1 - i, "none": lambda i: INT_MIN}
        live = [k for k, p in enumerate(plants) if p[1] == tz]
        assert [int(ref["assoc"][k]) for k in live] == [want[plants[k][6]](owners[k]) for k in live], (tz, ref["assoc"][:P])
        assert (np.delete(ref["assoc"], live) == INT_MIN).all()
        names = [plants[k][6] for k in live]
        assert counts_of(ref) == (800, len(live) - names.count("none"), names.count("range"), names.count("adopted") + names.count("kept") +
                                  names.count("conflict"), names.count("adopted"), names.count("kept"), names.count("conflict")), counts_of(ref)
        for k in live:
            name, _, rho, sig, mt, (dr, ds, dm), outcome = plants[k]
            i = owners[k]
            if outcome == "adopted":
                yz = 1.0 + np.float64(F32(rho)) * tz
                assert ref["prs4"][i, 2] == F32(np.float64(F32(rho)) / yz) and ref["prs4"][i, 3] < before[0][i, 3], name
                assert ref["matches"][i] == max(mt, dm), name
            else:
                assert ref["prs4"][i].tobytes() == before[0][i].tobytes() and ref["matches"][i] == before[1][i], name
        changed = np.flatnonzero((ref["prs4"] != before[0]).any(1) & ~np.isnan(before[0]).any(1))
        assert set(changed) == {owners[k] for k in live if plants[k][6] == "adopted"}


def test_a_successor_smaller_than_the_map(B, scene):
    """dst cut from a map of 300 keylines (the detection mask's doing): owners at or beyond 300 are not associated"""
    S = scene
    src, D = S.by_size[800]
    dst = successor(S, 5, size=300)
    ref = assert_handover(B, S, dst, src, D, *true_motion(), "dst 300")
    own = np.where(S.prop["assoc"] == INT_MIN, -1, np.where(S.prop["assoc"] < 0, -1 - S.prop["assoc"].astype(np.int64), S.prop["assoc"]))
    assert (own >= 300).sum() > 100 and (ref["assoc"][own >= 300] == INT_MIN).all() and (ref["assoc"][(own >= 0) & (own < 300)] != INT_MIN).all()
    assert ref["associated"] == int(((own >= 0) & (own < 300)).sum()) and ref["adopted"] > 20


def test_two_runs_are_byte_identical(B, scene):
    S = scene
    src, D = S.by_size[800]
    R, t = true_motion()
    outs = []
    for _ in range(2):
        dst = successor(S, 9)
        got, assoc = dst.handover_depth(src, S.mc, R, t, want_assoc=True)
        outs.append((bytes(got), assoc.tobytes(), *(x.tobytes() for x in dst.download())))
    assert outs[0] == outs[1] and counts_of(got)[4] > 100


def test_handover_over_the_capped_grid(B):
    """keylines_max = 65 536 on a 2304 x 1900 frame (the frame of the alignment's large case): both grids at their cap of 256
    workgroups; dst is the snapshot of the current map itself, with detection's raw depths - the caller's contract"""
    Wb, Hb = 2304, 1900
    frames, cam = enlarged_stream(Wb, Hb, 3)
    ctx = B.Context(B.default_params(Hb, Wb, fm=cam.fm, cx=cam.cx, cy=cam.cy, keylines_ref=60000, keylines_max=65536))
    maps = sorted((ctx.detect_u8(frames[i], i * 50000) for i in range(3)), key=lambda x: -x.size())
    mk, mc = maps[0], maps[1]
    assert mk.size() == 65536 and mc.size() > 32768
    kl, cur = current_data(mc)
    A = craft_against(kl, cur[2], cur[3], 5, cam_of(ctx))
    base = mk.keylines()
    base["matches"] = 0
    mk.upload(craft_kf_keylines(base, A, min(len(A["prs4"]), len(base))))
    src = mk.keyframe_snapshot()
    src.add_normals(mk)
    dst = mc.keyframe_snapshot()
    D = (cam_of(ctx), *src.download(), src.normals())
    ref = assert_handover(B, None, dst, src, D, *true_motion(), "large", mc=mc, ctx=ctx, cur=cur)
    print("large:", counts_of(ref))
    assert ref["candidates"] == 65536 and ref["associated"] > 32768
    slots = ref["assoc"][ref["assoc"] >= 0]
    assert (slots < 16384).sum() > 1000 and (slots >= mc.size() - 16384).sum() > 1000            # first and last workgroups of dst
    assert (ref["assoc"][:16384] >= 0).sum() > 1000 and (ref["assoc"][32768:] >= 0).sum() > 1000   # ...and of src
    src.release()
    dst.release()
    ctx.close()


# ---- 2. nothing to do; launches, resources, refusals -----------------------------------------------------------------------------------
def _small(B, n=65):
    """a fresh context of keylines_max n with a crafted src and the current map's own snapshot as dst"""
    frames, cam = stream()
    ctx = B.Context(params_for(B, cam, keylines_ref=max(1, n - 1), keylines_max=n, global_min_matches_threshold=1))
    mk, mc = [ctx.detect_u8(frames[1 + k], k * TS) for k in range(2)]
    assert mk.size() == n == mc.size()
    kl, cur = current_data(mc)
    A = craft_against(kl, cur[2], cur[3], 1, cam_of(ctx))
    base = mk.keylines()
    base["matches"] = 0
    mk.upload(craft_kf_keylines(base, A, min(len(A["prs4"]), n)))
    src = mk.keyframe_snapshot()
    src.add_normals(mk)
    return ctx, mk, mc, cur, src


def test_an_empty_src_launches_nothing(B):
    frames, cam = stream()
    ctx = B.Context(params_for(B, cam, **KW_STREAM))
    mk = ctx.detect_u8(np.full((H, W), 128, np.uint8), 0)
    mc = ctx.detect_u8(frames[1], TS)
    assert mk.size() == 0 and mc.size() > 0
    src, dst = mk.keyframe_snapshot(), mc.keyframe_snapshot()
    before = [x.tobytes() for x in dst.download()]
    base = B.test_live_resources()
    ctx.profile_reset()
    ctx.profile(True)
    got, assoc = dst.handover_depth(src, mc, *true_motion(), want_assoc=True)
    launches = {name: calls for name, (_, calls) in ctx.profile_read().items() if calls}
    ctx.profile(False)
    assert launches == {} and B.test_live_resources() == base, launches
    assert counts_of(got) == (0, 0, 0, 0, 0, 0, 0) and len(assoc) == 0
    assert [x.tobytes() for x in dst.download()] == before
    # an empty dst: every owner is beyond it
    got = src.handover_depth(dst, mc, *true_motion())
    assert counts_of(got) == (mc.size(), 0, 0, 0, 0, 0, 0)
    src.release()
    dst.release()
    ctx.close()


def test_the_entry_launches_what_it_documents(B):
    """two kernels per call; one allocation at the first call, kept"""
    ctx, mk, mc, cur, src = _small(B)
    dst = mc.keyframe_snapshot()
    src.download()
    dst.download()
    R, t = true_motion()
    base = B.test_live_resources()
    ctx.profile_reset()
    ctx.profile(True)
    dst.handover_depth(src, mc, R, t)
    launches = {name: calls for name, (_, calls) in ctx.profile_read().items() if calls}
    assert launches == dict(k_kf_handover_claim=1, k_kf_handover_apply=1), launches
    assert B.test_live_resources() == base + 1
    dst.handover_depth(src, mc, R, t, want_assoc=True)
    dst.handover_depth(src, mc, R, t)
    launches = {name: calls for name, (_, calls) in ctx.profile_read().items() if calls}
    ctx.profile(False)
    assert launches == dict(k_kf_handover_claim=3, k_kf_handover_apply=3), launches
    assert B.test_live_resources() == base + 1
    src.release()
    dst.release()
    ctx.close()


def test_refusals(B):
    frames, cam = stream()
    live = B.test_live_resources()
    ctx, other = B.Context(params_for(B, cam, **KW_STREAM)), B.Context(params_for(B, cam, **KW_STREAM))
    maps = [ctx.detect_u8(frames[k], k * TS) for k in range(3)]
    foreign = other.detect_u8(frames[0], 0)
    src, dst, fsnap = maps[0].keyframe_snapshot(), maps[1].keyframe_snapshot(), foreign.keyframe_snapshot()
    before = [x.tobytes() for s in (src, dst) for x in s.download()]
    L = B.lib()
    err = lambda: L.rebvio_hip_last_error().decode()
    out = B.KfHandover()
    dp = C.POINTER(C.c_double)
    R, t = np.eye(3), np.array([0.01, 0.0, 0.0])
    pR, pt = R.ctypes.data_as(dp), t.ctypes.data_as(dp)
    base = B.test_live_resources()
    ho = L.rebvio_hip_kf_snapshot_handover_depth
    m1 = maps[1].h
    assert ho(None, src.h, m1, None, pR, pt, C.byref(out), None) == -3 and "null" in err()
    assert ho(dst.h, None, m1, None, pR, pt, C.byref(out), None) == -3 and "null" in err()
    assert ho(dst.h, src.h, None, None, pR, pt, C.byref(out), None) == -3 and "null" in err()
    assert ho(dst.h, src.h, m1, None, None, pt, C.byref(out), None) == -3 and "null" in err()
    assert ho(dst.h, src.h, m1, None, pR, None, C.byref(out), None) == -3 and "null" in err()
    assert ho(dst.h, src.h, m1, None, pR, pt, None, None) == -3 and "null" in err()
    assert ho(dst.h, dst.h, m1, None, pR, pt, C.byref(out), None) == -3 and "same snapshot" in err()
    assert ho(fsnap.h, src.h, m1, None, pR, pt, C.byref(out), None) == -3 and "another context" in err()
    assert ho(dst.h, fsnap.h, m1, None, pR, pt, C.byref(out), None) == -3 and "another context" in err()
    assert ho(dst.h, src.h, foreign.h, None, pR, pt, C.byref(out), None) == -3 and "another context" in err()
    nan_R = np.eye(3)
    nan_R[2, 0] = np.nan
    sr = int(ctx.p.search_range)
    d = lambda **kw: dict(R=R, t=t, opts=B.default_kf_handover_opts(ctx, **kw))
    for kw, word in ((dict(R=nan_R, t=t), "non-finite"), (dict(R=R, t=[0.0, 0.0, -np.inf]), "non-finite"), (d(gate_sigma=0.0), "gate_sigma"),
                     (d(gate_sigma=float("nan")), "gate_sigma"), (d(q_abs=-1.0), "q_abs"), (d(q_abs=float("nan")), "q_abs"),
                     (d(min_cos=1.5), "min_cos"), (d(min_cos=-1.5), "min_cos"), (d(min_cos=float("nan")), "min_cos"), (d(max_dist=-1), "max_dist"),
                     (d(max_dist=sr + 1), "max_dist"), (d(reserved=2), "reserved"), (d(kf_filter=dict(rho_min=-1.0)), "rho_min"),
                     (d(kf_filter=dict(max_rel_sigma=float("nan"))), "NaN")):
        with pytest.raises(B.HipError) as e:
            dst.handover_depth(src, maps[1], **kw)
        assert "error -3:" in str(e.value) and word in str(e.value), (kw, str(e.value))
    assert B.test_live_resources() == base                      # nothing was allocated by a refused call
    assert B.default_kf_handover_opts(ctx).max_dist == sr
    # an uploaded map: its field is not detection's - refused
    maps[2].upload(maps[2].keylines())
    with pytest.raises(B.HipError, match="error -7:.*distance field"):
        dst.handover_depth(src, maps[2], R, t)
    assert [x.tobytes() for s in (src, dst) for x in s.download()] == before      # no refused call wrote a snapshot
    dst.handover_depth(src, maps[1], R, t, B.default_kf_handover_opts(ctx, max_dist=sr, min_cos=1.0, q_abs=0.0))      # the bounds themselves are legal
    assert B.test_live_resources() == base + 1
    ctx.close()
    assert ho(dst.h, src.h, m1, None, pR, pt, C.byref(out), None) == -10 and "destroyed" in err()
    assert ho(dst.h, src.h, foreign.h, None, pR, pt, C.byref(out), None) == -10 and "destroyed" in err()
    for s in (src, dst, fsnap):
        s.release()
    other.close()
    for m in maps + [foreign]:
        m.release()
    assert B.test_live_resources() == live


# ---- 3. with the tracker ----------------------------------------------------------------------------------------------------------------
def test_handover_calls_between_pairs_disturb_nothing(B):
    """the pair records and the final keylines of the stream are equal word for word with and without alignment and hand-over calls
    between the pairs"""
    frames, cam = stream()

    def run(with_handover):
        ctx = B.Context(params_for(B, cam, **KW_STREAM))
        maps = [ctx.detect_u8(frames[k], k * TS) for k in range(9)]
        recs, snap, R, t = [], None, None, None
        for k in range(8):
            out = ctx.track_pair(maps[k], maps[k + 1])
            recs.append(rec(out, maps[k + 1].size()))
            if k in (1, 4, 6):
                maps[k + 1].mark_keyframe()          # (marked in both runs: the ids are part of what is compared)
                if with_handover:
                    new = maps[k + 1].keyframe_snapshot()
                    new.add_normals(maps[k + 1])
                    if snap is not None:
                        got = maps[k + 1].keyframe_align(snap, None, R, t)
                        if got.status == 0:
                            h = new.handover_depth(snap, maps[k + 1], np.array(got.R), np.array(got.t))
                            print(f"mark at {k + 1}: aligned {got.used} of {got.candidates}; handed over {counts_of(h)}")
                            assert_identities(counts_of(h))
                        snap.release()
                    snap, R, t = new, None, None
            elif snap is not None and with_handover:
                got = maps[k + 1].keyframe_align(snap, None, R, t)
                if got.status == 0:
                    R, t = np.array(got.R), np.array(got.t)
                    snap.fuse_depth(maps[k + 1], R, t)
        final = maps[8].keylines()
        if snap:
            snap.release()
        ctx.close()
        return recs, final

    plain, kl_plain = run(False)
    handed, kl_handed = run(True)
    same_records(plain, handed, "with and without alignment, fusion and hand-over calls")
    assert kl_plain.tobytes() == kl_handed.tobytes()


# ---- the refusal table: every shared refusal with its code and whole text; which one wins when several apply ------

HAND = "kf_snapshot_handover_depth"
_ho = lambda dst, src, m, s, R="R", t="t", **kw: dst.handover_depth(src, m, getattr(s, R) if R else None, getattr(s, t) if t else None,
                                                                  s.B.default_kf_handover_opts(s.ctx, **kw) if kw else None)
REFUSED = {
    "destroyed map": (lambda s: _ho(s.dsnap, s.snap, s.dm, s), -10, DEAD_MAP),
    "destroyed successor": (lambda s: _ho(s.dsnap, s.snap, s.m2, s), -10, DEAD_SNAPSHOT),
    "destroyed source": (lambda s: _ho(s.snap2, s.dsnap, s.m2, s), -10, DEAD_SNAPSHOT),
    "foreign successor": (lambda s: _ho(s.fsnap, s.snap, s.m2, s), -3, foreign_snapshot(HAND)),
    "foreign source": (lambda s: _ho(s.snap2, s.fsnap, s.m2, s), -3, foreign_snapshot(HAND)),
    "no field": (lambda s: _ho(s.snap2, s.snap, s.up, s), -7, no_field(HAND)),
    "null R": (lambda s: _ho(s.snap2, s.snap, s.m2, s, R=None), -3, f"{HAND}: null R or t"),
    "R not finite": (lambda s: _ho(s.snap2, s.snap, s.m2, s, R="nan_R"), -3, f"{HAND}: non-finite R or t"),
    "t not finite": (lambda s: _ho(s.snap2, s.snap, s.m2, s, t="inf_t"), -3, f"{HAND}: non-finite R or t"),
    "gate_sigma": (lambda s: _ho(s.snap2, s.snap, s.m2, s, gate_sigma=0.0), -3, f"{HAND}: gate_sigma must be > 0"),
    "q_abs": (lambda s: _ho(s.snap2, s.snap, s.m2, s, q_abs=float("nan")), -3, f"{HAND}: q_abs must be >= 0"),
    "min_cos": (lambda s: _ho(s.snap2, s.snap, s.m2, s, min_cos=-1.5), -3, f"{HAND}: min_cos outside [-1, 1]"),
    "max_dist below": (lambda s: _ho(s.snap2, s.snap, s.m2, s, max_dist=-1), -3, f"{HAND}: max_dist outside 0..search_range"),
    "max_dist above": (lambda s: _ho(s.snap2, s.snap, s.m2, s, max_dist=s.sr + 1), -3, f"{HAND}: max_dist outside 0..search_range"),
    "wins: the successor, foreign, over the source, destroyed": (lambda s: _ho(s.fsnap, s.dsnap, s.m2, s), -3, foreign_snapshot(HAND)),
    "wins: the successor, destroyed, over the source, foreign": (lambda s: _ho(s.dsnap, s.fsnap, s.m2, s), -10, DEAD_SNAPSHOT),
    "wins: a foreign snapshot over a pose, an option and no field": (lambda s: _ho(s.snap2, s.fsnap, s.up, s, R="nan_R", gate_sigma=0.0), -3,
                                                                     foreign_snapshot(HAND)),
    "wins: a destroyed map over a foreign snapshot": (lambda s: _ho(s.snap2, s.snap, s.dm, s), -10, DEAD_MAP),
    "wins: the filter over the pose": (lambda s: _ho(s.snap2, s.snap, s.m2, s, R="nan_R", kf_filter=dict(rho_min=-1.0)), -3,
                                       f"{HAND}: filter rho_min must be > 0"),
    "wins: the pose over gate_sigma": (lambda s: _ho(s.snap2, s.snap, s.m2, s, t="inf_t", gate_sigma=0.0), -3, f"{HAND}: non-finite R or t"),
    "wins: gate_sigma over q_abs": (lambda s: _ho(s.snap2, s.snap, s.m2, s, gate_sigma=0.0, q_abs=-1.0), -3, f"{HAND}: gate_sigma must be > 0"),
    "wins: q_abs over min_cos": (lambda s: _ho(s.snap2, s.snap, s.m2, s, q_abs=-1.0, min_cos=2.0), -3, f"{HAND}: q_abs must be >= 0"),
    "wins: min_cos over max_dist": (lambda s: _ho(s.snap2, s.snap, s.m2, s, min_cos=2.0, max_dist=-1), -3, f"{HAND}: min_cos outside [-1, 1]"),
    "wins: max_dist over reserved": (lambda s: _ho(s.snap2, s.snap, s.m2, s, max_dist=-1, reserved=2), -3,
                                     f"{HAND}: max_dist outside 0..search_range"),
    "wins: an option over no field": (lambda s: _ho(s.snap2, s.snap, s.up, s, reserved=2), -3, f"{HAND}: reserved must be 0"),
}

@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusal_table(refusal_scene, case):
    """every refusal of the table with its return code and its whole rebvio_hip_last_error text; nothing is allocated"""
    assert_refused(refusal_scene, *REFUSED[case])
