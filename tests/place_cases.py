"""Crafted inputs of place recognition, shared by tests/test_place.py (hooks against the numpy restatement) and
tests/test_place_gpu.py (kernels against the hooks): keyline tables with keylines planted on every edge of the definition, random
tables with hostile values mixed in, database rows with extreme, tied and lane-boundary entries, a 65 536-row table whose top 16 is
known in closed form for 4096 queries that together name every row, the launch arithmetic of a query restated, and 17 000 rows
with ties and cuts planted in single threads' shares of k_place_topk's scan."""
import numpy as np

from rebvio_amd import backend as B

F32 = np.float32
NAN, INF = F32(np.nan), F32(np.inf)
SIZES = ((32, 32), (33, 37), (48, 96))   # (rows, cols): 37 columns are no multiple of 8, 33 rows none of 6
WORDS = 384


def keylines(n):
    """n keylines that count, all in word 0: pos (0, 0), gradient (1, 0)"""
    kl = np.zeros(n, B.KEYLINE_DTYPE)
    kl["gradient"] = (1.0, 0.0)
    kl["gradient_norm"] = 1.0
    kl["rho"], kl["sigma_rho"] = 1.0, 20.0
    kl["id"] = np.arange(n)
    return kl


def dn(v):
    return np.nextafter(F32(v), F32(-np.inf))


def planted(rows, cols):
    """One table with a keyline on every edge the definition has -> (keylines, names); its length does not depend on the values."""
    pos, grad, gn, names = [], [], [], []

    def add(name, p, g=(1.0, 0.0), n=1.0):
        pos.append(p), grad.append(g), gn.append(n), names.append(name)

    # pos exactly on every cell border and one ulp below it, along x and along y
    for c in range(8):
        x = -(-c * cols // 8)   # the first column of cell column c
        add(f"x border {c}", (F32(x), 1.0))
        add(f"x under border {c}", (dn(x), 1.0))
    for r in range(6):
        y = -(-r * rows // 6)
        add(f"y border {r}", (1.0, F32(y)))
        add(f"y under border {r}", (1.0, dn(y)))
    # the image's own borders and what lies outside
    for name, p in (("-0 x", (-0.0, 2.0)), ("-0 y", (2.0, -0.0)), ("-0 both", (-0.0, -0.0)), ("x = cols", (F32(cols), 2.0)),
                    ("y = rows", (2.0, F32(rows))), ("x under cols", (dn(cols), 2.0)), ("y under rows", (2.0, dn(rows))),
                    ("x negative", (-1.0, 2.0)), ("y negative", (2.0, -0.5)), ("x nan", (NAN, 2.0)), ("y nan", (2.0, NAN)),
                    ("x inf", (INF, 2.0)), ("y -inf", (2.0, -INF)), ("x huge", (F32(3e9), 2.0)), ("x fraction", (5.999, 7.001))):
        add(name, p)
    # signed zeros in the gradient; ties |gx| == |gy| in the four quadrants; each octant once
    for gx in (0.0, -0.0):
        for gy in (1.0, -1.0):
            add(f"gx {gx} gy {gy}", (3.0, 3.0), (gx, gy))
            add(f"gx {gy} gy {gx}", (3.0, 3.0), (gy, gx))
    for gx in (2.0, -2.0):
        for gy in (2.0, -2.0):
            add(f"tie {gx} {gy}", (4.0, 4.0), (gx, gy))
            add(f"octant x {gx} {gy}", (4.0, 4.0), (gx, gy / 2))
            add(f"octant y {gx} {gy}", (4.0, 4.0), (gx / 2, gy))
    add("tie one ulp", (4.0, 4.0), (2.0, np.nextafter(F32(2.0), INF)))
    add("denormal gradient", (4.0, 4.0), (F32(1e-45), 0.0))
    # gradients and norms that do not count
    for name, g in (("zero", (0.0, 0.0)), ("minus zero", (-0.0, -0.0)), ("gx inf", (INF, 1.0)), ("gy -inf", (1.0, -INF)), ("gx nan", (NAN, 1.0)),
                    ("gy nan", (1.0, NAN)), ("both nan", (NAN, NAN))):
        add("gradient " + name, (5.0, 5.0), g)
    for name, n in (("0", 0.0), ("-0", -0.0), ("negative", -1.0), ("nan", NAN), ("inf", INF), ("denormal", F32(1e-45))):
        add("norm " + name, (5.0, 5.0), (1.0, 0.0), n)
    kl = keylines(len(pos))
    kl["pos"] = np.array(pos, F32)
    kl["gradient"] = np.array(grad, F32)
    kl["gradient_norm"] = np.array(gn, F32)
    return kl, names


def random_table(rng, rows, cols, n, hostile=0.15):
    """n keylines over and around the image, a share of them with a value that must not count"""
    kl = keylines(n)
    if n == 0:
        return kl
    kl["pos"][:, 0] = rng.uniform(-2.0, cols + 2.0, n).astype(F32)
    kl["pos"][:, 1] = rng.uniform(-2.0, rows + 2.0, n).astype(F32)
    snap = rng.random(n) < 0.3          # whole pixels: the cell borders get hit
    kl["pos"][snap] = np.floor(kl["pos"][snap])
    g = rng.normal(0.0, 30.0, (n, 2)).astype(F32)
    tie = rng.random(n) < 0.1
    g[tie, 1] = g[tie, 0] * rng.choice([-1.0, 1.0], tie.sum()).astype(F32)
    kl["gradient"] = g
    kl["gradient_norm"] = np.hypot(g[:, 0], g[:, 1]).astype(F32)
    bad = np.flatnonzero(rng.random(n) < hostile)
    vals = np.array([NAN, INF, -INF, 0.0, -0.0], F32)
    for i in bad:
        f = rng.integers(0, 5)
        v = vals[rng.integers(0, len(vals))]
        if f < 2:
            kl["pos"][i, f] = v
        elif f < 4:
            kl["gradient"][i, f - 2] = v
        else:
            kl["gradient_norm"][i] = v
    return kl


def one_word(n, rows, cols):
    """n keylines in one word: its value is 65535"""
    kl = keylines(n)
    kl["pos"] = (cols - 1.0, rows - 1.0)
    kl["gradient"] = (-1.0, -3.0)
    return kl, 47 * 8 + 7


def three_words():
    """three keylines in three words: 21845 each"""
    kl = keylines(3)
    kl["gradient"] = [(1.0, 0.0), (-1.0, 0.0), (0.0, 1.0)]
    return kl, (0, 2, 1)


def db_rows(rng, n):
    """-> (rows uint16 [n, 384], query uint16 [384]): random full-range rows; from four rows on the first rows differ from the query
    in one word only - word 0, 5, 6 (the last of lane 0 and the first of lane 1) and 383 - by the same amount (a tie of four), with
    more rows an exact copy of the query (distance 0), a copy of that copy (a tie at 0), and the farthest row there is follow."""
    rows = rng.integers(0, 65536, (n, WORDS), dtype=np.uint16)
    q = rng.integers(0, 65536, WORDS, dtype=np.uint16)
    q[[0, 5, 6, 383]] = (100, 200, 300, 65535)
    if n >= 4:
        for r, w in enumerate((383, 6, 5, 0)):
            rows[r] = q
            rows[r, w] = q[w] - 7
    if n >= 63:
        rows[n - 2] = q
        rows[9] = q
        rows[n // 2] = np.where(q < 32768, 65535, 0).astype(np.uint16)
        rows[40] = rows[41] = rows[n - 1]   # ties among random rows
    return rows, q


# ---- a table in which every row is some query's answer ---------------------------------------------------------------------------
# Row i: every even word is 16 * (i // 16), every odd word (i % 16) + off[w]; query j: even words 16 * j, odd words off[w]. The 192
# even words differ by 16 * |i // 16 - j| each and the 192 odd words by i % 16 each: d(i) = 3072 * |i // 16 - j| + 192 * (i % 16).
# Block j holds 0, 192, ..., 2880, its neighbours start at 3072 (row r of block j - 1 ties with row r of block j + 1: the lower
# index first); at 65 536 eligible rows query j returns rows 16 j .. 16 j + 15, so the 4096 queries name every row once.
BLOCK_ROWS = 65536
BLOCK = 16


_BLOCK_OFF = np.random.default_rng(20250).integers(0, 60000, WORDS // 2).astype(np.uint16)
_BLOCK_OFF.setflags(write=False)


def block_offsets():
    """one offset per odd word, 0 .. 59 999: the lanes of k_place_dist hold different words, so a lane mix-up shows"""
    return _BLOCK_OFF


def block_table(n=BLOCK_ROWS):
    """-> rows uint16 [n, 384]; the largest word is 16 * 4095 = 65 520"""
    i = np.arange(n, dtype=np.int64)
    rows = np.empty((n, WORDS), np.uint16)
    rows[:, 0::2] = (BLOCK * (i // BLOCK))[:, None]
    rows[:, 1::2] = (i % BLOCK)[:, None] + block_offsets().astype(np.int64)[None, :]
    return rows


def block_query(j):
    q = np.empty(WORDS, np.uint16)
    q[0::2] = BLOCK * j
    q[1::2] = block_offsets()
    return q


def block_tag(i):
    return (1 << 40) + 3 * i


def block_top(eligible, j, k=16):
    """the closed form: [(distance, index)] of query j over the rows i < eligible, for a j whose block holds an eligible row. Blocks
    j - 2 .. j + 2 cut at `eligible` are enough: with j >= 1 block j - 1 is whole and no farther than 3072 + 2880, so with the row
    of block j there are 17 rows under the 3 * 3072 of every block outside; with j = 0 block 0 is either whole or all there is."""
    assert 0 <= BLOCK * j < eligible
    near = range(max(0, BLOCK * (j - 2)), min(eligible, BLOCK * (j + 3)))
    return sorted((3072 * abs(i // BLOCK - j) + 192 * (i % BLOCK), i) for i in near)[:k]


# ---- the launch arithmetic of a query, restated ---------------------------------------------------------------------------------
# track.hip: k_place_dist runs min(ceil(E / 4), kPlcDistBlocks) workgroups of four waves; wave w takes rows w, w + waves, ...,
# kPlcUnroll at a time while the last of the four is eligible, then one at a time. k_place_topk's plc_scan gives thread t of 1024
# the rows t, t + 1024, ..., eight per outer iteration.
PLC_DIST_BLOCKS = 2048   # kPlcDistBlocks
PLC_UNROLL = 4           # kPlcUnroll
PLC_TOPK_THREADS = 1024
PLC_SCAN_STEP = 8 * 1024

# the eligible counts the block-table tests run at; tests/test_place.py::test_launch_arithmetic_of_the_sizes asserts what each reaches
BLOCK_ELIGIBLE = (8188, 8189, 8192, 8193, 24576, 24577, 32768, 32769, 40000, 57344, 57345, 65535, 65536)


def dist_waves(eligible):
    return 4 * min(-(-eligible // 4), PLC_DIST_BLOCKS)


def dist_wave_shape(eligible, wave):
    """-> (unrolled passes, tail rounds, rows) of one wave of k_place_dist"""
    waves = dist_waves(eligible)
    e, passes, tail, rows = wave, 0, 0, []
    while e + (PLC_UNROLL - 1) * waves < eligible:
        rows += [e + u * waves for u in range(PLC_UNROLL)]
        passes, e = passes + 1, e + PLC_UNROLL * waves
    while e < eligible:
        rows.append(e)
        tail, e = tail + 1, e + waves
    return passes, tail, rows


def scan_shape(eligible, tid):
    """-> (outer iterations, rows) of thread tid in plc_scan"""
    return len(range(tid, eligible, PLC_SCAN_STEP)), len(range(tid, eligible, PLC_TOPK_THREADS))


# ---- rows for k_place_topk: one thread's rows over more than one outer iteration of its scan --------------------------------------
TOPK_ROWS = 17000   # thread t of 1024 owns rows t, t + 1024, ...: 17 of them for t < 616, 16 above; a scan takes 8 per iteration
TOPK_CASES = ("16-way tie of thread 5", "16-way tie of thread 1023", "distances falling with the index", "two owners alternating",
              "exclude_last through a group of eight", "the last row alone", "the last eligible row alone")


def topk_rows():
    """-> (rows uint16 [17000, 384], cases). Random rows with the rows of six cases planted among them, each case around a random
    query of its own, so that the rows of the other cases are as far from it as random rows are (about 384 * 21 845; the planted
    ones are within 16). cases: name -> (query, k, exclude_last, head), head = the first records by hand as [(distance, index)];
    what follows the head, if anything, are random rows and comes from the references."""
    rng = np.random.default_rng(1717)
    n = TOPK_ROWS
    rows = rng.integers(0, 65536, (n, WORDS), dtype=np.uint16)
    cases = {}

    def query():
        return rng.integers(1000, 60000, WORDS, dtype=np.uint16)

    def near(q, d):
        r = q.copy()
        r[int(rng.integers(0, WORDS))] += d    # one word, d above: distance d
        return r

    # sixteen copies of the query, all one thread's: a 16-way tie, won in index order by rescanning above the last winner
    for t in (5, 1023):
        q = query()
        own = [t + 1024 * u for u in range(16)]
        rows[own] = q
        cases[f"16-way tie of thread {t}"] = (q, 16, 0, [(0, i) for i in own])
    # the same thread's rows at distances that fall with u: the winners walk backwards through the owner's rows
    q = query()
    for u in range(16):
        rows[7 + 1024 * u] = near(q, 16 - u)
    cases["distances falling with the index"] = (q, 16, 0, [(16 - u, 7 + 1024 * u) for u in range(15, -1, -1)])
    # two owners taking turns in a tie
    q = query()
    own = [9 + (u & 1) + 1024 * u for u in range(16)]
    rows[own] = q
    cases["two owners alternating"] = (q, 16, 0, [(0, i) for i in own])
    # exclude_last cuts through one group of eight of thread 100's second scan iteration: rows 100 + 1024 u, u = 8 .. 15, are
    # copies; eligible = 100 + 1024 * 13, so u = 8 .. 12 count and u = 13 (the row AT eligible), 14 and 15 do not
    q = query()
    rows[[100 + 1024 * u for u in range(8, 16)]] = q
    eligible = 100 + 1024 * 13
    cases["exclude_last through a group of eight"] = (q, 16, n - eligible, [(0, 100 + 1024 * u) for u in range(8, 13)])
    # the last eligible row as the only match: the last row of all, and the last one in front of a cut that hides a copy behind it
    q = query()
    rows[n - 1] = q
    cases["the last row alone"] = (q, 16, 0, [(0, n - 1)])
    q = query()
    rows[[12345, 12346]] = q
    cases["the last eligible row alone"] = (q, 16, n - 12346, [(0, 12345)])
    assert tuple(cases) == TOPK_CASES
    return rows, cases


def extreme_rows():
    """the largest distance there is: all words 65535 against all words 0"""
    return np.full((1, WORDS), 65535, np.uint16), np.zeros(WORDS, np.uint16)
