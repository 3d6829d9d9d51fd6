"""Place recognition without a device: the ABI surface and its argument checks, the host hooks
(rebvio_hip_test_place_signature_host / _query_host: the statements of rebvio_amd/csrc/place.hpp, which the kernels run too) against
the numpy restatement of the header's definition (tests/place_ref.py) by equality, planted cases worked out by hand
(tests/place_cases.py), and what the signature buys on the CPU oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import place_cases as PC
import place_ref as R
from conftest import params_for
from support import KW_TRACK, ROOT, backend  # noqa: F401


def both(B, rows, cols, kl):
    """the hook and the restatement on one table, asserted equal in every word -> (sig, counted)"""
    sig, n = B.place_signature_host(rows, cols, kl)
    sig2, n2 = R.signature(rows, cols, kl)
    assert n == n2, (n, n2)
    assert sig.dtype == np.uint16 and np.array_equal(sig, sig2), np.flatnonzero(sig != sig2)[:8]
    return sig, n


def both_query(B, rows384, q, k, exclude_last=0):
    got = [(m.distance, m.index) for m in B.place_query_host(rows384, q, k, exclude_last)]
    assert all(m.tag == 0 for m in B.place_query_host(rows384, q, k, exclude_last))
    assert got == R.query(rows384, q, k, exclude_last), (got, R.query(rows384, q, k, exclude_last))
    return got


# ---- the ABI surface --------------------------------------------------------------------------------------------------------------
def test_layout_and_constants(backend):
    B = backend
    assert C.sizeof(B.PlaceMatch) == 16 and B.PlaceMatch.index.offset == 4 and B.PlaceMatch.tag.offset == 8
    assert (B.PLACE_WORDS, B.PLACE_TOPK_MAX) == (R.WORDS, R.TOPK_MAX) == (384, 16)
    text = open(os.path.join(ROOT, "include", "rebvio_hip.h")).read()
    assert "#define REBVIO_HIP_PLACE_WORDS 384" in text and "#define REBVIO_HIP_PLACE_TOPK_MAX 16" in text


def test_every_null_argument_is_refused_before_a_device_is_touched(backend):
    """-3 from every entry for null arguments, on a machine with or without a device"""
    L = backend.lib()
    sig = np.zeros(384, np.uint16)
    out = (backend.PlaceMatch * 16)()
    n, h, tag = C.c_int(), C.c_void_p(), C.c_uint64()
    s = sig.ctypes.data
    calls = [
        L.rebvio_hip_map_place_signature(None, s, C.byref(n)),
        L.rebvio_hip_place_db_create(None, 4, C.byref(h)),
        L.rebvio_hip_place_db_clear(None),
        L.rebvio_hip_place_db_size(None),
        L.rebvio_hip_place_db_add(None, None, 0, C.byref(n)),
        L.rebvio_hip_place_db_add_signature(None, s, 0, 0, C.byref(n)),
        L.rebvio_hip_place_db_entry(None, 0, s, C.byref(n), C.byref(tag)),
        L.rebvio_hip_place_db_query(None, None, 1, 0, out, C.byref(n)),
        L.rebvio_hip_place_db_query_signature(None, s, 1, 0, out, C.byref(n)),
    ]
    assert calls == [-3] * len(calls), calls
    assert not h.value
    L.rebvio_hip_place_db_release(None)   # (a no-op)


def test_the_hooks_refuse_bad_arguments(backend):
    B, L = backend, backend.lib()
    sig = np.zeros(384, np.uint16)
    rows = np.zeros((3, 384), np.uint16)
    kl = PC.keylines(2)
    out = (B.PlaceMatch * 16)()
    n = C.c_int()
    s, r, k = sig.ctypes.data, rows.ctypes.data, kl.ctypes.data
    bad = [
        L.rebvio_hip_test_place_signature_host(32, 32, k, 2, None, C.byref(n)),
        L.rebvio_hip_test_place_signature_host(32, 32, k, 2, s, None),
        L.rebvio_hip_test_place_signature_host(32, 32, None, 2, s, C.byref(n)),
        L.rebvio_hip_test_place_signature_host(32, 32, k, -1, s, C.byref(n)),
        L.rebvio_hip_test_place_signature_host(0, 32, k, 2, s, C.byref(n)),
        L.rebvio_hip_test_place_signature_host(32, 0, k, 2, s, C.byref(n)),
        L.rebvio_hip_test_place_query_host(None, 3, s, 1, 0, out, C.byref(n)),
        L.rebvio_hip_test_place_query_host(r, -1, s, 1, 0, out, C.byref(n)),
        L.rebvio_hip_test_place_query_host(r, 3, None, 1, 0, out, C.byref(n)),
        L.rebvio_hip_test_place_query_host(r, 3, s, 1, 0, None, C.byref(n)),
        L.rebvio_hip_test_place_query_host(r, 3, s, 1, 0, out, None),
        L.rebvio_hip_test_place_query_host(r, 3, s, 0, 0, out, C.byref(n)),
        L.rebvio_hip_test_place_query_host(r, 3, s, 17, 0, out, C.byref(n)),
        L.rebvio_hip_test_place_query_host(r, 3, s, -1, 0, out, C.byref(n)),
        L.rebvio_hip_test_place_query_host(r, 3, s, 1, -1, out, C.byref(n)),
    ]
    assert bad == [-3] * len(bad), bad
    assert L.rebvio_hip_test_place_signature_host(32, 32, None, 0, s, C.byref(n)) == 0 and n.value == 0
    assert L.rebvio_hip_test_place_query_host(None, 0, s, 1, 0, out, C.byref(n)) == 0 and n.value == 0


# ---- the signature -------------------------------------------------------------------------------------------------------------------
def test_signature_of_oracle_maps(backend, orc_mod, small_stream):
    frames, cam = small_stream
    orc = orc_mod.Oracle(params_for(orc_mod, cam, **KW_TRACK))
    seen = []
    for i in range(4):
        kl = orc.detect_u8(frames[i], i * 50000).keylines()
        sig, n = both(backend, cam.height, cam.width, kl)
        assert n == len(kl) > 300                    # every detected keyline counts
        assert 65535 - 384 < int(sig.astype(np.int64).sum()) <= 65535   # (each word rounds down by less than one)
        seen.append(sig)
    assert R.distance(seen[0], seen[1]) > 0


@pytest.mark.parametrize("rows,cols", [(33, 37), (48, 96)])
def test_signature_of_random_tables(backend, rows, cols):
    rng = np.random.default_rng(rows * 1000 + cols)
    counted = 0
    for t in range(200):
        n = int(rng.integers(0, 400))
        kl = PC.random_table(rng, rows, cols, n)
        sig, c = both(backend, rows, cols, kl)
        assert c <= n
        counted += c
    assert counted > 200 * 100


@pytest.mark.parametrize("rows,cols", PC.SIZES)
def test_planted_keylines(backend, rows, cols):
    B = backend
    kl, names = PC.planted(rows, cols)
    both(B, rows, cols, kl)
    word = {}
    for i, name in enumerate(names):      # each keyline alone: counted or not, and in which word
        sig, c = both(B, rows, cols, kl[i:i + 1])
        assert c in (0, 1) and int(sig.astype(np.int64).sum()) == 65535 * c, name
        word[name] = int(np.flatnonzero(sig)[0]) if c else None
    # by hand
    for c in range(8):
        assert word[f"x border {c}"] == c * 8, (c, word[f"x border {c}"])
        assert word[f"x under border {c}"] == ((c - 1) * 8 if c else None)
    for r in range(6):
        assert word[f"y border {r}"] == r * 64
        assert word[f"y under border {r}"] == ((r - 1) * 64 if r else None)
    assert word["-0 x"] == word["-0 y"] == word["-0 both"] == 0
    assert word["x under cols"] == 7 * 8 and word["y under rows"] == 5 * 64
    for name in ("x = cols", "y = rows", "x negative", "y negative", "x nan", "y nan", "x inf", "y -inf", "x huge"):
        assert word[name] is None, name
    cell = R.words_of(rows, cols, _at(3.0, 3.0))[0]
    # bin = 4 * (gy < 0) + 2 * (gx < 0) + (|gy| > |gx|); -0.0 is not negative
    assert word["gx 0.0 gy 1.0"] - cell == 1 and word["gx -0.0 gy 1.0"] - cell == 1
    assert word["gx 0.0 gy -1.0"] - cell == 5 and word["gx -0.0 gy -1.0"] - cell == 5
    assert word["gx 1.0 gy 0.0"] - cell == 0 and word["gx 1.0 gy -0.0"] - cell == 0
    assert word["gx -1.0 gy 0.0"] - cell == 2 and word["gx -1.0 gy -0.0"] - cell == 2
    cell = R.words_of(rows, cols, _at(4.0, 4.0))[0]
    for gx in (2.0, -2.0):
        for gy in (2.0, -2.0):
            base = 4 * (gy < 0) + 2 * (gx < 0)
            assert word[f"tie {gx} {gy}"] - cell == base
            assert word[f"octant x {gx} {gy}"] - cell == base
            assert word[f"octant y {gx} {gy}"] - cell == base + 1
    assert word["tie one ulp"] - cell == 1 and word["denormal gradient"] - cell == 0
    for name in names:
        if name.startswith("gradient "):
            assert word[name] is None, name
    assert [word["norm " + n] is None for n in ("0", "-0", "negative", "nan", "inf", "denormal")] == [True, True, True, True, False, False]


def _at(x, y):
    kl = PC.keylines(1)
    kl["pos"] = (x, y)
    kl["gradient"] = (1.0, 0.0)
    return kl


def test_normalisation_by_hand(backend):
    B = backend
    sig, n = both(B, 33, 37, PC.keylines(0))
    assert n == 0 and not sig.any()
    dead = PC.keylines(5)
    dead["gradient_norm"] = 0.0
    sig, n = both(B, 33, 37, dead)
    assert n == 0 and not sig.any()
    for count in (1, 2, 255, 65536):
        kl, w = PC.one_word(count, 33, 37)
        sig, n = both(B, 33, 37, kl)
        assert n == count and sig[w] == 65535 and int(sig.astype(np.int64).sum()) == 65535, count
    kl, ws = PC.three_words()
    sig, n = both(B, 33, 37, kl)
    assert n == 3 and [int(sig[w]) for w in ws] == [21845] * 3 and int(sig.astype(np.int64).sum()) == 3 * 21845
    # a keyline that does not count changes nothing
    more = np.concatenate([kl, dead])
    assert np.array_equal(both(B, 33, 37, more)[0], sig)


# ---- the query -----------------------------------------------------------------------------------------------------------------------
def test_query_extremes_ties_and_k(backend):
    B = backend
    rows, q = PC.extreme_rows()
    assert both_query(B, rows, q, 1) == [(384 * 65535, 0)] and R.D_MAX == 384 * 65535
    assert both_query(B, rows, rows[0], 3) == [(0, 0)]
    rng = np.random.default_rng(5)
    for n in (1, 3, 4, 5, 63, 64, 65, 257):
        rows, q = PC.db_rows(rng, n)
        for k in (1, 2, 16):
            got = both_query(B, rows, q, k)
            assert len(got) == min(k, n)
            assert got == sorted(got)
        if n >= 4:
            got = both_query(B, rows, q, 16)
            if n >= 63:   # the two copies tie at 0 (lower index first), then the four one-word rows tie at 7
                assert got[:6] == [(0, 9), (0, n - 2), (7, 0), (7, 1), (7, 2), (7, 3)], got[:6]
                far = R.query(rows, q, 16)  # (the farthest row is none of the nearest)
                assert n // 2 not in [e for _, e in far]
                assert R.distance(rows[n // 2], q) == int(np.maximum(q.astype(np.int64), 65535 - q.astype(np.int64)).sum())
            else:
                assert got[:4] == [(7, 0), (7, 1), (7, 2), (7, 3)], got[:4]
        # exclude_last: up to, at and past the size
        for ex in (1, n - 1, n, n + 5):
            got = both_query(B, rows, q, 16, ex)
            assert len(got) == min(16, max(0, n - ex)) and all(e < n - ex for _, e in got)


def test_query_rows_differing_in_one_word(backend):
    """a row that differs from the query in word 0, 5, 6 or 383 only - the first and last word of lane 0, the first of lane 1, the
    last of lane 63 - is at exactly that difference"""
    B = backend
    rng = np.random.default_rng(6)
    q = rng.integers(1000, 60000, 384, dtype=np.uint16)
    rows = np.repeat(q[None, :], 9, 0)
    for r, (w, d) in enumerate(((0, 1), (5, 2), (6, 3), (383, 4), (0, -5), (5, -6), (6, -7), (383, -8))):
        rows[r, w] = int(q[w]) + d
    got = both_query(B, rows, q, 9)
    assert got == [(0, 8)] + [(r + 1, r) for r in range(8)], got


# ---- the block table: every row is some query's answer --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def block_rows():
    rows = PC.block_table()
    rows.setflags(write=False)
    return rows


def _blocks_to_try(eligible):
    last = (eligible - 1) // PC.BLOCK
    return sorted({j for j in (0, 1, last // 2, last - 1, last) if 0 <= j <= last})


def test_block_table_closed_form_against_the_restatement(block_rows):
    """the closed form of tests/place_cases.py equals place_ref.query at every eligible count the GPU tests use (and at 17, inside
    the second block), for the first two blocks, a middle one and the last two - the last is cut wherever the count is no multiple
    of 16 - and every row is in the top 16 of its own block's query: the queries together name every eligible row"""
    assert block_rows.shape == (65536, 384) and int(block_rows.max()) == 65520
    assert len(np.unique(block_rows[:, :2].astype(np.int64) @ np.array([65536, 1]))) == 65536   # the first two words name the row
    for eligible in (17,) + PC.BLOCK_ELIGIBLE:
        ex = PC.BLOCK_ROWS - eligible
        for j in _blocks_to_try(eligible):
            want = R.query(block_rows, PC.block_query(j), 16, ex)
            assert PC.block_top(eligible, j) == want, (eligible, j, PC.block_top(eligible, j), want)
            for k in (1, 4):
                assert PC.block_top(eligible, j, k) == want[:k]
        named = set()
        for j in range(-(-eligible // PC.BLOCK)):
            named.update(i for _, i in PC.block_top(eligible, j))
        assert named == set(range(eligible)), eligible
    full = PC.block_top(65536, 4095)
    assert full == [(192 * r, 65520 + r) for r in range(16)]
    assert PC.block_top(8189, 511) == [(192 * r, 8176 + r) for r in range(13)] + [(3072 + 192 * r, 8160 + r) for r in range(3)]
    assert PC.block_top(17, 1)[:3] == [(0, 16), (3072, 0), (3264, 1)]


@pytest.mark.parametrize("eligible,j", [(65536, 4095), (65535, 4095), (24577, 1536), (8193, 512), (40000, 1234)])
def test_block_table_closed_form_against_the_hook(backend, block_rows, eligible, j):
    """a handful only: the hook recomputes every distance in every round"""
    got = backend.place_query_host(block_rows, PC.block_query(j), 16, PC.BLOCK_ROWS - eligible)
    assert [(m.distance, m.index) for m in got] == PC.block_top(eligible, j)


def test_launch_arithmetic_of_the_sizes():
    """what each eligible count of the block-table tests reaches in k_place_dist (waves; unrolled passes and tail rounds of wave 0
    and of the last wave) and in plc_scan (outer iterations), from the restatement of the launch arithmetic in
    tests/place_cases.py: kPlcDistBlocks = 2048, kPlcUnroll = 4, plc_scan's 8 * 1024"""
    assert (PC.PLC_DIST_BLOCKS, PC.PLC_UNROLL, PC.PLC_SCAN_STEP) == (2048, 4, 8 * 1024)
    text = open(os.path.join(ROOT, "rebvio_amd", "csrc", "track.hip")).read()
    assert "constexpr int kPlcUnroll = 4;" in text and "constexpr int kPlcDistBlocks = 2048;" in text
    assert "for (int e = tid; e < eligible; e += 8 * 1024)" in text and "__launch_bounds__(1024) void k_place_topk" in text

    def shape(eligible):
        waves = PC.dist_waves(eligible)
        first, last = PC.dist_wave_shape(eligible, 0)[:2], PC.dist_wave_shape(eligible, waves - 1)[:2]
        return waves, first, last

    # every row is some wave's, once
    for eligible in PC.BLOCK_ELIGIBLE + (4200, PC.TOPK_ROWS):
        waves = PC.dist_waves(eligible)
        seen = np.zeros(eligible, np.int64)
        for w in range(waves):
            np.add.at(seen, PC.dist_wave_shape(eligible, w)[2], 1)
        assert (seen == 1).all(), eligible
    # what the suite had: 4200 rows are as many rows as waves - one row per wave through the tail loop, no stride, no unrolled pass -
    # and at most five rows per thread of k_place_topk in one outer iteration
    assert shape(4200) == (4200, (0, 1), (0, 1)) and PC.scan_shape(4200, 0) == (1, 5) and PC.scan_shape(4200, 1023) == (1, 4)
    # the cap of 2048 workgroups: 2047 of them, then 2048 with the last three waves idle
    assert shape(8188) == (8188, (0, 1), (0, 1))
    assert shape(8189) == (8192, (0, 1), (0, 0))
    # the last size with one row per wave; then the tail loop's first stride and plc_scan's first second iteration, thread 0 alone
    assert shape(8192) == (8192, (0, 1), (0, 1)) and PC.scan_shape(8192, 0) == (1, 8)
    assert shape(8193) == (8192, (0, 2), (0, 1))
    assert PC.scan_shape(8193, 0) == (2, 9) and PC.scan_shape(8193, 1) == (1, 8)
    # three tail rounds and no unrolled pass; then wave 0 alone takes one, over rows 0, 8192, 16 384, 24 576
    assert shape(24576) == (8192, (0, 3), (0, 3))
    assert shape(24577) == (8192, (1, 0), (0, 3)) and PC.dist_wave_shape(24577, 0)[2] == [0, 8192, 16384, 24576]
    assert PC.dist_wave_shape(24577, 1)[:2] == (0, 3)
    # exactly one unrolled pass each and no tail; plus one tail row
    assert shape(32768) == (8192, (1, 0), (1, 0))
    assert shape(32769) == (8192, (1, 1), (1, 0))
    # one unrolled pass, a tail for the waves below 7232 only
    assert shape(40000) == (8192, (1, 1), (1, 0))
    assert PC.dist_wave_shape(40000, 7231)[:2] == (1, 1) and PC.dist_wave_shape(40000, 7232)[:2] == (1, 0)
    # the second unrolled pass begins
    assert shape(57344) == (8192, (1, 3), (1, 3))
    assert shape(57345) == (8192, (2, 0), (1, 3))
    # the envelope: at 65 535 the last wave falls out of its second pass into three tail rounds
    assert shape(65535) == (8192, (2, 0), (1, 3))
    assert shape(65536) == (8192, (2, 0), (2, 0))
    assert PC.scan_shape(65536, 0) == PC.scan_shape(65536, 1023) == (8, 64)
    assert PC.scan_shape(65535, 1023) == (8, 63)
    # the top-k table: thread 5 scans 17 rows in three outer iterations, thread 1023 16 rows in two
    assert PC.scan_shape(PC.TOPK_ROWS, 5) == (3, 17) and PC.scan_shape(PC.TOPK_ROWS, 1023) == (2, 16)
    assert PC.scan_shape(PC.TOPK_ROWS, 615) == (3, 17) and PC.scan_shape(PC.TOPK_ROWS, 616) == (2, 16)
    assert shape(PC.TOPK_ROWS) == (8192, (0, 3), (0, 2))


def test_topk_cases_by_hand_and_against_both_references(backend):
    """the rows planted for k_place_topk (tests/place_cases.py::topk_rows): the hook and the restatement agree on every record and
    begin with the records stated by hand; what follows a head is a random row, far away"""
    rows, cases = PC.topk_rows()
    assert rows.shape == (PC.TOPK_ROWS, 384) and len(cases) == 7
    for name, (q, k, ex, head) in cases.items():
        got = both_query(backend, rows, q, k, ex)
        assert got[:len(head)] == head, (name, got, head)
        assert len(got) == 16 and all(i < PC.TOPK_ROWS - ex for _, i in got), name
        assert all(d > 1000000 for d, _ in got[len(head):]), (name, got)
        for kk in (1, 4):
            assert both_query(backend, rows, q, kk, ex) == got[:kk], name
    # the row at the cut and the copies behind it exist and are not eligible
    q, k, ex, head = cases["exclude_last through a group of eight"]
    eligible = PC.TOPK_ROWS - ex
    assert eligible == 100 + 1024 * 13 and all(np.array_equal(rows[100 + 1024 * u], q) for u in range(8, 16))
    q, k, ex, head = cases["the last eligible row alone"]
    assert np.array_equal(rows[PC.TOPK_ROWS - ex], q) and head == [(0, PC.TOPK_ROWS - ex - 1)]


# ---- what it buys --------------------------------------------------------------------------------------------------------------------
def _oracle_sigs(orc_mod, backend, cam, scene, ts, seed_add):
    """signatures of the maps a fresh oracle, warmed by three detections of its first frame, detects at the times ts"""
    from rebvio_amd import synth
    orc = orc_mod.Oracle(params_for(orc_mod, cam, **KW_TRACK))
    frames = [synth.render_frame(scene, cam, float(t), noise_seed=int(10 * t) + seed_add) for t in ts]
    for i in range(3):
        orc.detect_u8(frames[0], i * 50000)
    out = []
    for i, f in enumerate(frames):
        kl = orc.detect_u8(f, (3 + i) * 50000).keylines()
        out.append(both(backend, cam.height, cam.width, kl)[0])
    return np.array(out)


def test_value_on_the_oracle(backend, orc_mod):
    """Scene 0 at 192x144 rendered at t = 0, 3, ..., 93 makes a database of 32 entries about 6 pixels apart. 11 queries at
    t = 3k + 1, k = 0, 3, ..., 30, under other noise and from another oracle: the nearest entry is k for every one of them, and
    twice the largest distance to a true entry stays under the smallest distance from four maps of scene 1 to any entry.
    Measured with this restatement: d_true 15 285 .. 21 846, the runner-up of those queries 22 698 .. 27 754 (entry k + 1 every
    time), the median over the database 74 330 .. 80 295, scene 1 (at t = 0, 30, 60, 90) no nearer than 72 978. The bound is the
    issue's, not a measurement: a true match may be twice as far as the farthest seen and still be nearer than another scene."""
    from rebvio_amd import synth
    cam = synth.Camera.for_size(192, 144)
    scene0, scene1 = synth.make_scene(0), synth.make_scene(1)
    db = _oracle_sigs(orc_mod, backend, cam, scene0, [3.0 * j for j in range(32)], 0)
    ks = list(range(0, 31, 3))
    qs = _oracle_sigs(orc_mod, backend, cam, scene0, [3.0 * k + 1.0 for k in ks], 555)
    d_true, d_next, med = [], [], []
    for k, q in zip(ks, qs):
        got = both_query(backend, db, q, 2)
        print("query", k, "->", got, "median", int(np.median([R.distance(r, q) for r in db])))
        assert got[0][1] == k, (k, got)
        d_true.append(got[0][0]), d_next.append(got[1][0]), med.append(int(np.median([R.distance(r, q) for r in db])))
    other = _oracle_sigs(orc_mod, backend, cam, scene1, [0.0, 30.0, 60.0, 90.0], 0)
    d_other = [both_query(backend, db, q, 1)[0][0] for q in other]
    print("d_true", min(d_true), max(d_true), "next", min(d_next), max(d_next), "median", min(med), max(med), "other scene", d_other)
    assert 2 * max(d_true) <= min(d_other), (max(d_true), min(d_other))
