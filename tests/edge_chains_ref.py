"""The numpy restatement of the edge chains and polylines (include/rebvio_hip.h is the definition): a plain sequential walk of each
path from its head and of each remaining cycle from its smallest member, then the chain table and the lines slot by slot. Checked
by hand in tests/test_edge_chains.py; the hooks and the device are compared with it by equality of integer arrays and record bytes.
Also the crafted link tables and keyline maps more than one test file uses."""
import numpy as np

from support import CLOUD_DTYPE, F32, np_cloud, np_passes

CHAIN_REF_DTYPE = np.dtype([("head", "<i4"), ("rank", "<i4"), ("length", "<i4"), ("flags", "<i4")])
POLYLINE_DTYPE = np.dtype([("first_point", "<i4"), ("points", "<i4"), ("head", "<i4"), ("flags", "<i4")])
DEFAULT_FILTER = (2, 0.5, 1e-3, 20.0)
WIDE = (0, 1e9, 1e-3, 20.0)           # every keyline with a rho inside the clamp passes
ENTRIES = ("rebvio_hip_map_edge_chains", "rebvio_hip_default_polyline_opts", "rebvio_hip_map_edge_polylines",
           "rebvio_hip_test_edge_chains_host", "rebvio_hip_test_edge_polylines_host")
KERNELS_CHAINS = ("k_chain_link", "k_chain_round", "k_chain_rank", "k_chain_count", "k_chain_emit", "k_chain_order")
KERNELS_POLY = ("k_poly_count", "k_poly_emit", "k_poly_lines")


def rounds_of(keylines_max):
    """ceil(log2(keylines_max)): the k_chain_round launches of a context"""
    r = 0
    while (1 << r) < keylines_max:
        r += 1
    return r


def np_succ(id_prev, id_next):
    idp, idn = np.asarray(id_prev, np.int64), np.asarray(id_next, np.int64)
    n = len(idp)
    succ = np.full(n, -1, np.int64)
    for i in range(n):
        s = int(idn[i])
        if 0 <= s < n and s != i and int(idp[s]) == i:
            succ[i] = s
    return succ


def np_chains(id_prev, id_next):
    """(refs CHAIN_REF_DTYPE [n], order int32 [n], starts int32 [C + 1], C)"""
    succ = np_succ(id_prev, id_next)
    n = len(succ)
    pred = np.full(n, -1, np.int64)
    for i in range(n):
        if succ[i] >= 0:
            assert pred[succ[i]] == -1          # pred is unique
            pred[succ[i]] = i
    refs = np.zeros(n, CHAIN_REF_DTYPE)
    seen = np.zeros(n, bool)
    chains = []                                  # (head, members in rank order)
    for h in range(n):                           # paths, each from its head
        if pred[h] != -1:
            continue
        members, i = [], h
        while i != -1:
            assert not seen[i]
            seen[i] = True
            members.append(i)
            i = int(succ[i])
        chains.append((h, members, 0))
    for h in range(n):                           # what is left lies on cycles; the first unseen member is the smallest
        if seen[h]:
            continue
        members, i = [], h
        while not seen[i]:
            seen[i] = True
            members.append(i)
            i = int(succ[i])
        assert i == h and min(members) == h
        chains.append((h, members, 1))
    chains.sort(key=lambda c: c[0])
    order = np.zeros(n, np.int32)
    starts = np.zeros(len(chains) + 1, np.int32)
    at = 0
    for c, (h, members, cyc) in enumerate(chains):
        starts[c] = at
        for r, i in enumerate(members):
            refs[i] = (h, r, len(members), cyc)
            order[at + r] = i
        at += len(members)
    starts[len(chains)] = n
    assert at == n
    return refs, order, starts, len(chains)


def np_polylines(kl, fm, flt=DEFAULT_FILTER, min_chain_length=8, pose=None):
    """(points CLOUD_DTYPE, refs2 int32 [k, 2], lines POLYLINE_DTYPE): the kept slots in slot order, each point the record np_cloud
    gives its keyline, and the maximal runs of kept consecutive slots of one chain (no wrap)."""
    refs, order, starts, C = np_chains(kl["id_prev"], kl["id_next"])
    cloud = np_cloud(kl, fm, flt, pose)
    rec_of = {int(k): j for j, k in enumerate(cloud["keyline"])}
    passes = np_passes(kl, *flt)
    pts, refs2, lines = [], [], []
    for c in range(C):
        slots = range(int(starts[c]), int(starts[c + 1]))
        length = len(slots)
        cyc = int(refs[order[slots[0]]]["flags"]) & 1
        run = None
        for s in slots:
            k = int(order[s])
            kept = bool(passes[k]) and length >= min_chain_length
            if kept:
                if run is None:
                    run = [len(pts), 0, int(refs[k]["head"]), 0]
                pts.append(cloud[rec_of[k]])
                refs2.append((int(refs[k]["head"]), int(refs[k]["rank"])))
                run[1] += 1
            if run is not None and (not kept or s == slots[-1]):
                run[3] = 1 if cyc and run[1] == length else 0
                lines.append(tuple(run))
                run = None
    points = np.array(pts, CLOUD_DTYPE) if pts else np.zeros(0, CLOUD_DTYPE)
    return points, np.array(refs2, np.int32).reshape(-1, 2), np.array(lines, POLYLINE_DTYPE) if lines else np.zeros(0, POLYLINE_DTYPE)


# ---- comparison: equality of integer arrays and of record bytes --------------------------------------------------------------
def assert_chains_equal(got, want, what=""):
    """got = (refs, order, starts, n_keylines, n_chains) of an entry or a hook; want = np_chains()"""
    refs, order, starts, nk, nc = got
    wrefs, worder, wstarts, wc = want
    assert (nk, nc) == (len(wrefs), wc), (what, nk, nc, len(wrefs), wc)
    assert refs.tobytes() == wrefs.tobytes(), (what, np.flatnonzero(refs != wrefs)[:8])
    assert np.array_equal(order, worder) and np.array_equal(starts, wstarts), what
    assert np.array_equal(np.sort(order), np.arange(nk)), what


def assert_polylines_equal(got, want, what=""):
    """got = (points, refs2, lines, n_points, n_lines) of an entry or a hook; want = np_polylines()"""
    pts, refs2, lines, npts, nl = got
    wpts, wrefs2, wlines = want
    assert (npts, nl) == (len(wpts), len(wlines)), (what, npts, nl, len(wpts), len(wlines))
    assert pts.tobytes() == wpts.tobytes() and np.array_equal(refs2, wrefs2) and lines.tobytes() == wlines.tobytes(), what


# ---- crafted link tables: (id_prev, id_next) int32 ------------------------------------------------------------------------
def links_of_sequences(n, paths=(), cycles=()):
    """id_prev / id_next (-1 elsewhere) that link every sequence of `paths` as a path and every one of `cycles` as a cycle"""
    idp, idn = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    for seq in paths:
        for a, b in zip(seq[:-1], seq[1:]):
            idn[a], idp[b] = b, a
    for seq in cycles:
        for a, b in zip(seq, list(seq[1:]) + [seq[0]]):
            idn[a], idp[b] = b, a
    return idp, idn


def dirty_links():
    """the hand cases of one table, n = 12: a path 0>1>2, a reversed path 5>4>3, a 2-cycle 6<>7, two claimants of one id_next (8 and 9
    both name 10; id_prev[10] keeps 9), an out-of-range link at 10 and a self link at 11"""
    idp = np.array([-1, 0, 1, 4, 5, -1, 7, 6, -1, -1, 9, 11], np.int32)
    idn = np.array([1, 2, -1, -1, 3, 4, 7, 6, 10, 10, 1000, 11], np.int32)
    return idp, idn


def shuffled_path(n, seed):
    perm = np.random.default_rng(seed).permutation(n)
    return links_of_sequences(n, paths=[list(perm)])


def random_links(rng, n):
    """arbitrary integers in both fields: mostly near-valid indices (so that links, claimants and cycles form), some far outside"""
    def field():
        v = rng.integers(-2, n + 2, n)
        wild = rng.random(n) < 0.1
        v[wild] = rng.choice(np.array([-2**31, 2**31 - 1, -1, n, 2 * n + 7, -n - 1]), int(wild.sum()))
        return v.astype(np.int32)
    idp, idn = field(), field()
    fix = rng.random(n) < 0.6                  # answer most id_next links so that chains longer than one link exist
    for i in np.flatnonzero(fix):
        s = int(idn[i])
        if 0 <= s < n:
            idp[s] = i
    if n >= 6 and rng.random() < 0.5:          # closed contours are rare in such a draw: plant one of 2..5 members
        seq = rng.choice(n, int(rng.integers(2, 6)), replace=False)
        for a, b in zip(seq, np.roll(seq, -1)):
            idn[a], idp[b] = b, a
    return idp, idn


def keylines_with_links(dtype, idp, idn, seed=0, rho=1.0):
    """keylines that pass the default filter everywhere (matches 3, sigma 0.05 rho) with distinct pos_img and gradient_norm"""
    n = len(idp)
    rng = np.random.default_rng(seed)
    kl = np.zeros(n, dtype)
    kl["pos_img"] = rng.uniform(-60, 60, (n, 2)).astype(F32)
    kl["pos"] = kl["pos_img"] + F32(80)
    kl["rho"] = (F32(rho) * rng.uniform(0.5, 1.5, n)).astype(F32)
    kl["sigma_rho"] = (F32(0.05) * kl["rho"]).astype(F32)
    kl["gradient"] = rng.uniform(-3, 3, (n, 2)).astype(F32)
    kl["gradient_norm"] = rng.uniform(1, 9, n).astype(F32)
    kl["matches"] = 3
    kl["id"] = np.arange(n)
    kl["id_prev"], kl["id_next"] = idp, idn
    kl["match_id"] = kl["match_id_forward"] = kl["match_id_keyframe"] = -1
    return kl


def planted_polyline_map(dtype):
    """n = 64: chain A = path 0..19 with filter failures planted at ranks 6 and 13 (three lines of 6, 6, 6); chain B = path 20..24 (5 <
    min_chain_length 8: nothing); chain C = cycle 25..36, all kept (one closed line of 12); chain D = cycle 37..48 with a failure at
    rank 0 (one open line of 11); chain E = cycle 49..63 with a failure at rank 7 (two open lines of 7 and 7: no wrap)."""
    idp, idn = links_of_sequences(64, paths=[list(range(0, 20)), list(range(20, 25))],
                                  cycles=[list(range(25, 37)), list(range(37, 49)), list(range(49, 64))])
    kl = keylines_with_links(dtype, idp, idn, seed=5)
    for k in (6, 13, 37, 56):
        kl["matches"][k] = 0
    want_lines = np.array([(0, 6, 0, 0), (6, 6, 0, 0), (12, 6, 0, 0), (18, 12, 25, 1), (30, 11, 37, 0), (41, 7, 49, 0), (48, 7, 49, 0)],
                          POLYLINE_DTYPE)
    return kl, want_lines
