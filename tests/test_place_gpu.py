"""Place recognition on the GPU: k_place_hist / k_place_norm / k_place_dist / k_place_topk against the host hooks, by equality.

Maps are crafted through rebvio_hip_map_upload (a context of keylines_max = n detects exactly n keylines on a checkerboard frame; the
upload then replaces them), database rows are planted through rebvio_hip_place_db_add_signature. Every word the device leaves - the
384 signature words, counted, each result record - is compared with the hooks (rebvio_hip_test_place_signature_host / _query_host,
the same statements), which tests/test_place.py holds against the numpy restatement of the header. The tests at the end run where
the kernels' loops iterate - databases of 8188 .. 65 536 eligible rows against a closed form that names every row, 17 000 rows with
ties planted inside one thread's share of k_place_topk, a map of 65 536 keylines."""
import ctypes as C
import time

import numpy as np
import pytest

import place_cases as PC
import place_ref as R
from conftest import params_for
from support import B, refusal_scene  # noqa: F401
from support import DEAD_MAP, DEAD_PLACE_DB, assert_refused, assert_release_keeps_the_message
from support import F32, KW_TRACK, noise_frames, vision_only_fusion

pytestmark = pytest.mark.gpu


def checker(rows, cols):
    """6-pixel checkerboard: 299 keylines at 32x32 with the threshold below, enough for maps of 257"""
    y, x = np.mgrid[0:rows, 0:cols]
    return ((((x // 6) + (y // 6)) % 2) * 200 + 20).astype(np.uint8)


def sized_ctx(B, n, rows=32, cols=32):
    from rebvio_amd import synth
    cam = synth.Camera.for_size(cols, rows)
    return B.Context(params_for(B, cam, keylines_ref=max(1, n - 1), keylines_max=max(1, n), threshold=0.001, gain=0.0,
                                global_min_matches_threshold=1))


def sized_map(ctx, n, ts=0):
    rows, cols = ctx.rows, ctx.cols
    m = ctx.detect_u8(checker(rows, cols) if n else np.full((rows, cols), 128, np.uint8), ts)
    assert m.size() == n, (m.size(), n)
    return m


def check_signature(B, m, kl, what=""):
    """upload kl, compare the device's signature with the hook's -> (sig, counted)"""
    ctx = m.ctx
    m.upload(kl)
    back = m.keylines()
    for f in ("pos", "gradient", "gradient_norm"):
        assert back[f].tobytes() == kl[f].tobytes(), (what, f)
    want, want_n = B.place_signature_host(ctx.rows, ctx.cols, back)
    got, got_n = m.place_signature()
    assert got_n == want_n, (what, got_n, want_n)
    assert np.array_equal(got, want), (what, np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8])
    after = m.keylines()
    assert after.tobytes() == back.tobytes(), what      # the map's keylines are untouched
    return got, got_n


def as_pairs(matches):
    return [(m.distance, m.index) for m in matches]


# ---- the signature -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", PC.SIZES)
def test_map_sizes_and_planted_keylines(B, rows, cols):
    """maps of 0, 1, 63, 64, 65, 256, 257 keylines (around a wave and a workgroup of k_place_hist) with hostile values mixed in, the
    planted table, all keylines in one word, three keylines in three words"""
    rng = np.random.default_rng(rows + cols)
    planted, _ = PC.planted(rows, cols)
    total = 0
    for n in (0, 1, 63, 64, 65, 256, 257, len(planted)):
        ctx = sized_ctx(B, n, rows, cols)
        m = sized_map(ctx, n)
        tables = [PC.random_table(rng, rows, cols, n), PC.random_table(rng, rows, cols, n, hostile=0.0)]
        if n == len(planted):
            tables.append(planted)
        tables.append(PC.one_word(n, rows, cols)[0])
        for t, kl in enumerate(tables):
            sig, c = check_signature(B, m, kl, what=f"{n} keylines, table {t}")
            total += c
        if n:
            sig, c = m.place_signature()                                     # (the last table: one word)
            assert c == n and sig[PC.one_word(n, rows, cols)[1]] == 65535 and int(sig.astype(np.int64).sum()) == 65535
        else:
            assert m.place_signature()[1] == 0 and not m.place_signature()[0].any()
        m.release()
        ctx.close()
    assert total > 1000
    ctx = sized_ctx(B, 3, rows, cols)
    m = sized_map(ctx, 3)
    kl, ws = PC.three_words()
    sig, c = check_signature(B, m, kl)
    assert c == 3 and [int(sig[w]) for w in ws] == [21845] * 3
    ctx.close()


def test_a_detected_map_against_numpy(B):
    from rebvio_amd import synth
    frames, cam = synth.render_stream(160, 120, 2)
    ctx = B.Context(params_for(B, cam, keylines_ref=600, keylines_max=800))
    for i in range(2):
        m = ctx.detect_u8(frames[i], i * 50000)
        kl = m.keylines()
        want, want_n = R.signature(cam.height, cam.width, kl)
        got, got_n = m.place_signature()
        assert got_n == want_n == len(kl) > 300
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    ctx.close()


def test_a_map_promised_to_r_prior_next_is_refused(B, small_stream):
    frames, cam = small_stream
    ctx = B.Context(params_for(B, cam, **KW_TRACK))
    maps = [ctx.detect_u8(frames[i], i * 50000) for i in range(2)]
    db = ctx.place_db(4)
    c, s = F32(np.cos(0.01)), F32(np.sin(0.01))
    Rn = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], F32)
    assert maps[1].place_signature()[1] == maps[1].size()
    mid = ctx.track_pair_begin(maps[0], maps[1])
    ctx.track_pair_finish_async(maps[0], maps[1], *vision_only_fusion(mid), R_prior_next=Rn)
    ctx.track_pair_result()
    for call in (lambda: maps[1].place_signature(), lambda: db.add(maps[1], 1), lambda: db.query(maps[1], 1)):
        with pytest.raises(B.HipError) as e:
            call()
        assert "error -7:" in str(e.value) and "R_prior_next" in str(e.value), str(e.value)
    assert db.size() == 0
    assert maps[0].place_signature()[1] == maps[0].size()      # an old map: the signature is of what it holds now
    ctx.close()


# ---- the database --------------------------------------------------------------------------------------------------------------------
def test_a_queued_add_equals_the_signature(B):
    rng = np.random.default_rng(3)
    ctx = sized_ctx(B, 257, 33, 37)
    m = sized_map(ctx, 257)
    db = ctx.place_db(3)
    want = []
    for t in range(3):
        kl = PC.random_table(rng, 33, 37, 257)
        m.upload(kl)
        before = m.keylines().tobytes()
        assert db.add(m, tag=1000 + t) == t and db.size() == t + 1
        want.append(m.place_signature())
        assert m.keylines().tobytes() == before
    for t in range(3):
        sig, counted, tag = db.entry(t)
        assert np.array_equal(sig, want[t][0]) and counted == want[t][1] and tag == 1000 + t, t
    assert not np.array_equal(want[0][0], want[1][0])
    with pytest.raises(B.HipError) as e:
        db.add(m, tag=9)
    assert "error -7:" in str(e.value) and "full" in str(e.value)
    assert db.size() == 3
    # the last map against its own database: itself at distance 0; from the map and from its signature alike
    got = db.query(m, 3)
    assert as_pairs(got) == as_pairs(db.query_signature(want[2][0], 3)) and [x.tag for x in got] == [x.tag for x in db.query_signature(want[2][0], 3)]
    assert as_pairs(got)[0] == (0, 2) and got[0].tag == 1002
    assert as_pairs(db.query(m, 3, exclude_last=1))[0][1] != 2
    db.release()
    ctx.close()


@pytest.mark.parametrize("cap", [1, 2, 65, 300])
def test_database_geometry(B, cap):
    """capacities around a wave and above a workgroup of k_place_topk's scan; databases of 1, 3, 4, 5, 63, 64, 65, 257 rows with the
    extreme, tied and lane-boundary rows; k at 1, 2, 16 and above the eligible count; exclude_last up to and past the size"""
    rng = np.random.default_rng(cap)
    ctx = sized_ctx(B, 1)
    db = ctx.place_db(cap)
    assert db.size() == 0 and db.query_signature(np.zeros(384, np.uint16), 16) == []
    for n in (1, 3, 4, 5, 63, 64, 65, 257):
        if n > cap:
            continue
        db.clear()
        assert db.size() == 0
        rows, q = PC.db_rows(rng, n)
        for i in range(n):
            assert db.add_signature(rows[i], counted=i, tag=(1 << 40) + i) == i
        assert db.size() == n
        for i in (0, n // 2, n - 1):
            sig, counted, tag = db.entry(i)
            assert np.array_equal(sig, rows[i]) and counted == i and tag == (1 << 40) + i
        for k in (1, 2, 16):
            for ex in (0, 1, n - 1, n, n + 5):
                got = db.query_signature(q, k, ex)
                want = B.place_query_host(rows, q, k, ex)
                assert as_pairs(got) == as_pairs(want), (n, k, ex, as_pairs(got), as_pairs(want))
                assert [m.tag for m in got] == [(1 << 40) + m.index for m in want]
                assert len(got) == min(k, max(0, n - ex))
        if n >= 63:
            assert as_pairs(db.query_signature(q, 16))[:6] == [(0, 9), (0, n - 2), (7, 0), (7, 1), (7, 2), (7, 3)]
    if db.size() == cap:
        with pytest.raises(B.HipError) as e:
            db.add_signature(np.zeros(384, np.uint16))
        assert "error -7:" in str(e.value)
    # the largest distance there is, and distance 0
    db.clear()
    rows, q = PC.extreme_rows()
    db.add_signature(rows[0])
    assert as_pairs(db.query_signature(q, 1)) == [(384 * 65535, 0)] and as_pairs(db.query_signature(rows[0], 16)) == [(0, 0)]
    db.release()
    ctx.close()


def test_rows_differing_in_one_word_and_many_rows(B):
    """word 0, 5, 6 and 383 - the ends of lane 0, the start of lane 1, the end of lane 63; then 4200 rows: 1050 workgroups of
    k_place_dist, so as many waves as rows - one row per wave, through the tail loop, which never takes its stride, and no pass of
    the unrolled loop - and up to five rows per thread of k_place_topk, in one outer iteration of its scan. The sizes at which
    those loops iterate are the block-table and top-k tests at the end of this file."""
    rng = np.random.default_rng(6)
    ctx = sized_ctx(B, 1)
    db = ctx.place_db(4200)
    q = rng.integers(1000, 60000, 384, dtype=np.uint16)
    rows = np.repeat(q[None, :], 9, 0)
    for r, (w, d) in enumerate(((0, 1), (5, 2), (6, 3), (383, 4), (0, -5), (5, -6), (6, -7), (383, -8))):
        rows[r, w] = int(q[w]) + d
    for r in rows:
        db.add_signature(r)
    assert as_pairs(db.query_signature(q, 9)) == [(0, 8)] + [(r + 1, r) for r in range(8)]
    db.clear()
    rows = rng.integers(0, 65536, (4200, 384), dtype=np.uint16)
    rows[4100] = rows[77]                     # a tie far apart
    rows[3000] = q
    for i, r in enumerate(rows):
        db.add_signature(r, tag=i)
    for k, ex in ((16, 0), (16, 1199), (3, 4190)):
        got, want = db.query_signature(q, k, ex), B.place_query_host(rows, q, k, ex)
        assert as_pairs(got) == as_pairs(want) and [m.tag for m in got] == [m.index for m in want], (k, ex)
    got = as_pairs(db.query_signature(rows[77], 2))
    assert got == [(0, 77), (0, 4100)], got
    db.release()
    ctx.close()


def test_every_minus_3_with_a_database(B):
    L = B.lib()
    ctx, other = sized_ctx(B, 3), sized_ctx(B, 3)
    m, mo = sized_map(ctx, 3), sized_map(other, 3)
    base = B.test_live_resources()
    h = C.c_void_p()
    for cap in (0, -1, 65537):
        assert L.rebvio_hip_place_db_create(ctx.h, cap, C.byref(h)) == -3 and not h.value
    assert L.rebvio_hip_place_db_create(ctx.h, 4, None) == -3
    assert B.test_live_resources() == base
    db = ctx.place_db(4)
    assert B.test_live_resources() == base + 2          # the rows; the distances, counted words and results
    sig = np.zeros(384, np.uint16)
    s = sig.ctypes.data
    out = (B.PlaceMatch * 16)()
    n, tag = C.c_int(), C.c_uint64()
    db.add_signature(sig)
    bad = [
        L.rebvio_hip_place_db_add(db.h, None, 0, None),
        L.rebvio_hip_place_db_add(db.h, mo.h, 0, None),                       # a map of another context
        L.rebvio_hip_place_db_add_signature(db.h, None, 0, 0, None),
        L.rebvio_hip_place_db_add_signature(db.h, s, -1, 0, None),
        L.rebvio_hip_place_db_entry(db.h, -1, s, C.byref(n), C.byref(tag)),
        L.rebvio_hip_place_db_entry(db.h, 1, s, C.byref(n), C.byref(tag)),    # index == size
        L.rebvio_hip_place_db_query(db.h, None, 1, 0, out, C.byref(n)),
        L.rebvio_hip_place_db_query(db.h, mo.h, 1, 0, out, C.byref(n)),
        L.rebvio_hip_place_db_query(db.h, m.h, 0, 0, out, C.byref(n)),
        L.rebvio_hip_place_db_query(db.h, m.h, 17, 0, out, C.byref(n)),
        L.rebvio_hip_place_db_query(db.h, m.h, 1, -1, out, C.byref(n)),
        L.rebvio_hip_place_db_query(db.h, m.h, 1, 0, None, C.byref(n)),
        L.rebvio_hip_place_db_query(db.h, m.h, 1, 0, out, None),
        L.rebvio_hip_place_db_query_signature(db.h, None, 1, 0, out, C.byref(n)),
        L.rebvio_hip_place_db_query_signature(db.h, s, 0, 0, out, C.byref(n)),
        L.rebvio_hip_place_db_query_signature(db.h, s, 17, 0, out, C.byref(n)),
        L.rebvio_hip_place_db_query_signature(db.h, s, 1, -1, out, C.byref(n)),
        L.rebvio_hip_map_place_signature(m.h, None, C.byref(n)),
        L.rebvio_hip_map_place_signature(m.h, s, None),
    ]
    assert bad == [-3] * len(bad), bad
    assert db.size() == 1
    assert L.rebvio_hip_place_db_entry(db.h, 0, None, None, None) == 0     # every output is optional
    assert B.test_live_resources() == base + 2                             # no refused call allocated anything
    db.release()
    ctx.close()
    other.close()


def test_launches_and_lifetime(B):
    """a signature is k_place_hist + k_place_norm, a query adds k_place_dist + k_place_topk, whatever the sizes; an empty eligible set
    launches nothing; the first signature gives the context one live resource, a database two; everything returns to its start
    after release, and after destroy followed by release (-10 from the husk in between)"""
    live = B.test_live_resources()
    ctx = sized_ctx(B, 257)
    m, m0 = sized_map(ctx, 257, 0), sized_map(ctx, 0, 50000)
    for x in (m, m0):
        x.keylines()
    base = B.test_live_resources()
    db = ctx.place_db(65)
    assert B.test_live_resources() == base + 2
    ctx.profile(True)

    def launches(call):
        ctx.profile_reset()
        call()
        return {name: calls for name, (_, calls) in ctx.profile_read().items() if calls}

    sig_only = {"k_place_hist": 1, "k_place_norm": 1}
    full = dict(sig_only, k_place_dist=1, k_place_topk=1)
    assert launches(lambda: db.query(m, 4)) == {}                      # an empty database
    assert B.test_live_resources() == base + 2
    assert launches(lambda: m.place_signature()) == sig_only
    assert B.test_live_resources() == base + 3
    assert launches(lambda: m0.place_signature()) == sig_only
    assert launches(lambda: (db.add(m, 1), db.entry(0))) == sig_only
    assert launches(lambda: db.query(m, 16, exclude_last=1)) == {}
    assert launches(lambda: db.query(m, 16)) == full
    assert launches(lambda: db.query(m0, 1)) == full
    assert launches(lambda: db.query_signature(np.zeros(384, np.uint16), 2)) == {"k_place_dist": 1, "k_place_topk": 1}
    for i in range(64):
        db.add(m0, i)
    assert launches(lambda: db.query(m, 16)) == full
    assert B.test_live_resources() == base + 3
    ctx.profile(False)
    db.release()
    assert B.test_live_resources() == base + 1
    db2, db3 = ctx.place_db(2), ctx.place_db(300)
    db2.add(m, 5)
    assert B.test_live_resources() == base + 5
    db3.release()
    ctx.close()                                                        # the database outlives its context as a husk
    L = B.lib()
    n = C.c_int()
    out = (B.PlaceMatch * 16)()
    sig = np.zeros(384, np.uint16)
    assert L.rebvio_hip_place_db_size(db2.h) == -10 and L.rebvio_hip_place_db_clear(db2.h) == -10
    assert L.rebvio_hip_place_db_entry(db2.h, 0, None, C.byref(n), None) == -10
    assert L.rebvio_hip_place_db_add_signature(db2.h, sig.ctypes.data, 0, 0, None) == -10
    assert L.rebvio_hip_place_db_query_signature(db2.h, sig.ctypes.data, 1, 0, out, C.byref(n)) == -10
    assert L.rebvio_hip_place_db_add(db2.h, m.h, 0, None) == -10 and L.rebvio_hip_place_db_query(db2.h, m.h, 1, 0, out, C.byref(n)) == -10
    db2.release()
    for x in (m, m0):
        x.release()
    assert B.test_live_resources() == live


# ---- where the query's loops iterate: up to 65 536 rows -------------------------------------------------------------------------------
def as_records(matches):
    return [(m.distance, m.index, m.tag) for m in matches]


@pytest.fixture(scope="module")
def block_db(B):
    """one database of capacity 65 536 holding tests/place_cases.py's block table; a test chooses the eligible count through
    exclude_last, so one fill serves every size"""
    ctx = sized_ctx(B, 1)
    db = ctx.place_db(PC.BLOCK_ROWS)
    rows = PC.block_table()
    t0 = time.perf_counter()
    for i in range(PC.BLOCK_ROWS):
        db.add_signature(rows[i], counted=i, tag=PC.block_tag(i))
    print(f"block_db: {PC.BLOCK_ROWS} add_signature calls in {time.perf_counter() - t0:.2f} s")
    assert db.size() == PC.BLOCK_ROWS
    for i in (0, 8191, 8192, 40000, 65535):
        sig, counted, tag = db.entry(i)
        assert np.array_equal(sig, rows[i]) and counted == i and tag == PC.block_tag(i), i
    yield db
    db.release()
    ctx.close()


def sweep_blocks(db, eligible, blocks, k=16):
    ex = PC.BLOCK_ROWS - eligible
    for j in blocks:
        got = as_records(db.query_signature(PC.block_query(j), k, ex))
        want = [(d, i, PC.block_tag(i)) for d, i in PC.block_top(eligible, j, k)]
        assert got == want, (eligible, j, k, got, want)


def test_every_row_of_a_full_database(B, block_db):
    """65 536 eligible rows: every wave of k_place_dist takes two unrolled passes and no tail, every thread of k_place_topk scans 64
    rows in eight outer iterations. The 4096 queries of the block table return every row once - distance, index and tag of every
    record against the closed form - so a wrong dist[e] of any row shows."""
    waves = PC.dist_waves(65536)
    assert waves == 8192 and PC.dist_wave_shape(65536, 0)[:2] == PC.dist_wave_shape(65536, waves - 1)[:2] == (2, 0)
    named = []
    for j in range(4096):
        got = as_records(block_db.query_signature(PC.block_query(j), 16))
        assert got == [(192 * r, 16 * j + r, PC.block_tag(16 * j + r)) for r in range(16)], (j, got)
        assert [(d, i) for d, i, _ in got] == PC.block_top(65536, j)
        named += [i for _, i, _ in got]
    assert named == list(range(65536))


@pytest.mark.parametrize("eligible", [e for e in PC.BLOCK_ELIGIBLE if e != 65536])
def test_every_eligible_row_at_the_sizes_where_the_loops_change(B, block_db, eligible):
    """the eligible counts of tests/place_cases.py::BLOCK_ELIGIBLE (what each reaches in k_place_dist and plc_scan is asserted by
    tests/test_place.py::test_launch_arithmetic_of_the_sizes): every query whose block holds an eligible row, every record against
    the closed form; at the first, a middle and the last two blocks k = 1 and k = 4 return the prefix of k = 16"""
    last = (eligible - 1) // PC.BLOCK
    sweep_blocks(block_db, eligible, range(last + 1))
    for k in (1, 4):
        sweep_blocks(block_db, eligible, sorted({0, last // 2, last - 1, last}), k)
    # no row at or past the cut comes back, whatever is asked
    for j in (last, min(last + 1, 4095), 4095):
        got = block_db.query_signature(PC.block_query(j), 16, PC.BLOCK_ROWS - eligible)
        assert len(got) == 16 and all(m.index < eligible for m in got), (eligible, j)


@pytest.fixture(scope="module")
def topk_db(B):
    ctx = sized_ctx(B, 1)
    db = ctx.place_db(PC.TOPK_ROWS)
    rows, cases = PC.topk_rows()
    for i in range(PC.TOPK_ROWS):
        db.add_signature(rows[i], tag=PC.block_tag(i))
    want = {name: B.place_query_host(rows, q, k, ex) for name, (q, k, ex, _) in cases.items()}   # once, for every test below
    yield db, cases, want
    db.release()
    ctx.close()


@pytest.mark.parametrize("name", PC.TOPK_CASES)
def test_one_thread_wins_round_after_round(B, topk_db, name):
    """17 000 rows: thread t of k_place_topk owns 16 or 17 rows over two or three outer iterations of plc_scan. The planted rows of
    tests/place_cases.py::topk_rows - a 16-way tie owned by thread 5 and by thread 1023, which must win 16 rounds in a row by
    scanning above its own last winner; distances falling with the index, so that the winners walk backwards through the owner's
    rows; two owners alternating in a tie; exclude_last cutting through one group of eight, the copy at the cut and the two behind
    it not returned; the last (eligible) row as the only match - every record against the hook and against the list by hand"""
    db, cases, hook = topk_db
    q, k, ex, head = cases[name]
    got = db.query_signature(q, k, ex)
    want = hook[name]
    assert as_pairs(got) == as_pairs(want), (name, as_pairs(got), as_pairs(want))
    assert [m.tag for m in got] == [PC.block_tag(m.index) for m in want]
    assert as_pairs(got)[:len(head)] == head, (name, as_pairs(got), head)
    assert len(got) == 16 and all(m.index < PC.TOPK_ROWS - ex for m in got)
    for kk in (1, 4):
        assert as_pairs(db.query_signature(q, kk, ex)) == as_pairs(got)[:kk], (name, kk)


def test_signature_at_the_envelope_of_65536_keylines(B):
    """keylines_max = 65 536 on a 640 x 896 noise frame: 256 workgroups of k_place_hist add into one global histogram. The detected
    keylines as they come, a random table with hostile values, all 65 536 in one word (every workgroup's full LDS count into one
    global word), 65 535 in one word and one in another ((65535 * 65535) // 65536 = 65534 and 65535 // 65536 = 0), one keyline
    of 65 536 uncounted; then maps of the same context that hold few and no keylines, where the workgroups past the size add nothing.
    Every word against the hook and against the numpy restatement."""
    rows, cols = 640, 896
    ctx = B.Context(B.default_params(rows, cols, fm=500.0, cx=447.5, cy=319.5, keylines_ref=60000, keylines_max=65536))
    m = ctx.detect_u8(noise_frames(cols, rows, 1, 3)[0], 0)
    assert m.size() == 65536

    def against_numpy(m, kl, what):
        want, want_n = R.signature(rows, cols, kl)
        got, got_n = m.place_signature()
        assert got_n == want_n, (what, got_n, want_n)
        assert np.array_equal(got, want), (what, np.flatnonzero(got != want)[:8])
        return got, got_n

    kl = m.keylines()
    sig, n = check_signature(B, m, kl, "detected")
    against_numpy(m, kl, "detected")
    assert n == 65536 and np.count_nonzero(sig) > 256
    rng = np.random.default_rng(65536)
    kl = PC.random_table(rng, rows, cols, 65536)
    sig, n = check_signature(B, m, kl, "random table")
    against_numpy(m, kl, "random table")
    assert 40000 < n < 65536 and np.count_nonzero(sig) == 384
    # by hand
    kl, w = PC.one_word(65536, rows, cols)
    sig, n = check_signature(B, m, kl, "one word")
    assert n == 65536 and sig[w] == 65535 and np.count_nonzero(sig) == 1
    two = kl.copy()
    two["pos"][40000] = (0.0, 0.0)
    two["gradient"][40000] = (1.0, 0.0)
    sig, n = check_signature(B, m, two, "65535 and 1")
    against_numpy(m, two, "65535 and 1")
    assert n == 65536 and sig[w] == 65534 and sig[0] == 0 and np.count_nonzero(sig) == 1
    for dead in (0, 255, 256, 65535):
        one = kl.copy()
        one["gradient_norm"][dead] = 0.0
        sig, n = check_signature(B, m, one, f"keyline {dead} uncounted")
        assert n == 65535 and sig[w] == 65535 and np.count_nonzero(sig) == 1
    # the same context, maps well under its keylines_max
    step = np.full((rows, cols), 20, np.uint8)
    step[:, cols // 2:] = 220
    sizes = []
    for ts, frame in ((50000, step), (100000, np.full((rows, cols), 128, np.uint8))):
        few = ctx.detect_u8(frame, ts)
        kl = few.keylines()
        sizes.append(len(kl))
        assert len(kl) == few.size() < 65536 - 256
        want, want_n = B.place_signature_host(rows, cols, kl)
        got, got_n = against_numpy(few, kl, f"{len(kl)} keylines")
        assert got_n == want_n and np.array_equal(got, want)
        few.release()
    assert sizes[0] > 256 and sizes[1] == 0 and got_n == 0 and not got.any(), sizes   # (one edge down the middle: about 1300)
    m.release()
    ctx.close()


# ---- the refusal table: every shared refusal with its code and whole text; which one wins when several apply ------

_sig = lambda: np.zeros(384, np.uint16)
_other = lambda who: f"{who}: map of another context than the database's"
REFUSED = {
    "clear": (lambda s: s.ddb.clear(), -10, DEAD_PLACE_DB),
    "size": (lambda s: s.B.lib().rebvio_hip_place_db_size(s.ddb.h), -10, DEAD_PLACE_DB),
    "add_signature": (lambda s: s.ddb.add_signature(_sig()), -10, DEAD_PLACE_DB),
    "entry": (lambda s: s.ddb.entry(0), -10, DEAD_PLACE_DB),
    "query_signature": (lambda s: s.ddb.query_signature(_sig()), -10, DEAD_PLACE_DB),
    "add: destroyed map": (lambda s: s.ddb.add(s.dm), -10, DEAD_MAP),
    "add: destroyed database": (lambda s: s.ddb.add(s.m), -10, DEAD_PLACE_DB),
    "add: foreign database": (lambda s: s.fdb.add(s.m), -3, _other("place_db_add")),
    "query: destroyed map": (lambda s: s.ddb.query(s.dm), -10, DEAD_MAP),
    "query: destroyed database": (lambda s: s.ddb.query(s.m), -10, DEAD_PLACE_DB),
    "query: foreign database": (lambda s: s.fdb.query(s.m), -3, _other("place_db_query")),
    "signature: destroyed map": (lambda s: s.dm.place_signature(), -10, DEAD_MAP),
    "wins: k over a destroyed database": (lambda s: s.ddb.query(s.m, k=0), -3, "place_db_query: k outside 1..16"),
    "wins: k over a destroyed database, by signature": (lambda s: s.ddb.query_signature(_sig(), k=17), -3,
                                                        "place_db_query_signature: k outside 1..16"),
    "wins: a destroyed database over the index": (lambda s: s.ddb.entry(-1), -10, DEAD_PLACE_DB),
    "wins: a destroyed map over a foreign database": (lambda s: s.db.add(s.dm), -10, DEAD_MAP),
}

@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusal_table(refusal_scene, case):
    """every refusal of the table with its return code and its whole rebvio_hip_last_error text; nothing is allocated"""
    assert_refused(refusal_scene, *REFUSED[case])


def test_releasing_a_database_leaves_the_last_error_alone(B):
    """rebvio_hip_place_db_release, of a husk and of a live database, writes no message"""
    assert_release_keeps_the_message(B, lambda ctx: ctx.place_db(4))
