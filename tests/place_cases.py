"""Crafted inputs of place recognition, shared by tests/test_place.py (hooks against the numpy restatement) and
tests/test_place_gpu.py (kernels against the hooks): keyline tables with keylines planted on every edge of the definition, random
tables with hostile values mixed in, and database rows with extreme, tied and lane-boundary entries."""
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


def extreme_rows():
    """the largest distance there is: all words 65535 against all words 0"""
    return np.full((1, WORDS), 65535, np.uint16), np.zeros(WORDS, np.uint16)
