"""Crafted inputs of the stereo prior, shared by tests/test_stereo_prior.py (hook against restatement) and
tests/test_stereo_prior_gpu.py (kernel against hook): right "maps" planted by hand - a keyline table and the dense mask that names
each keyline at its cell - and left keylines whose outcome follows from the header's text by hand.

Geometry of the planted cases: fm = 80, baseline = 0.125, so fb = 10 exactly and rho_m = d / 10. A left keyline at (x, y) with
gradient (1, 0) and a right keyline at (x - d, y) with the same gradient give xr = x - d and the disparity d without rounding."""
import numpy as np

from rebvio_amd import backend as B

F32 = np.float32
NAN = F32(np.nan)
FM, BASE = 80.0, 0.125
ROWS, COLS = 48, 96


def keylines(n, rho=1.0, sigma=20.0):
    kl = np.zeros(n, B.KEYLINE_DTYPE)
    kl["rho"], kl["sigma_rho"] = F32(rho), F32(sigma)
    kl["gradient"] = (1.0, 0.0)
    kl["gradient_norm"] = 1.0
    kl["id"] = np.arange(n)
    return kl


def plant(rows, cols, entries):
    """entries: (cell x, cell y, pos x, pos y, gx, gy, gn) per right keyline, j = its index -> (keylines, mask int32 [rows, cols])"""
    kr = keylines(len(entries))
    mask = np.full((rows, cols), -1, np.int32)
    for j, (cx, cy, x, y, gx, gy, gn) in enumerate(entries):
        kr["pos"][j] = (x, y)
        kr["gradient"][j] = (gx, gy)
        kr["gradient_norm"][j] = gn
        assert mask[cy, cx] == -1
        mask[cy, cx] = j
    return kr, mask


def at(x, y, gx=1.0, gy=0.0, gn=1.0):
    """a right keyline whose cell is the one its position rounds to"""
    return (int(np.floor(x + 0.5)), int(np.floor(y + 0.5)), x, y, gx, gy, gn)


def planted_cases():
    """-> list of (name, rows, cols, fm, left, right, mask, opts, expected outcome words, expected winners or None)"""
    up, dn = lambda v, to=np.inf: np.nextafter(F32(v), F32(to)), lambda v: np.nextafter(F32(v), F32(-np.inf))  # noqa: E731
    out = []

    def case(name, left, entries, want, win=None, rows=ROWS, cols=COLS, fm=FM, **opts):
        kr, mask = plant(rows, cols, entries)
        out.append((name, rows, cols, fm, left, kr, mask, dict(dict(baseline=BASE), **opts), want, win))

    # no direction; |ux| exactly at min_ux and one ulp under it (the right keyline shares the gradient, so it passes where asked)
    h = F32(0.75) ** F32(0.5)
    kl = keylines(7)
    kl["pos"] = [(40.0, 3.0 * i + 2) for i in range(7)]
    kl["gradient_norm"][:4] = (0.0, NAN, -1.0, 1.0)
    kl["gradient"][3] = (np.inf, 0.0)
    kl["gradient"][4] = (0.5, h)
    kl["gradient"][5] = (dn(0.5), h)
    kl["gradient"][6] = (-0.5, h)
    ent = [at(35.0, 3.0 * i + 2) for i in range(4)] + [at(35.0, 14.0, 0.5, h), at(35.0, 17.0, 0.5, h), at(35.0, 20.0, -0.5, h)]
    case("direction", kl, ent, [3, 3, 3, 3, 1, 3, 1], [-1, -1, -1, -1, 4, -1, 6], row_tol=0)

    # the image's borders with row_tol = 1: column 0 (its partner sits left of the image's first pixel centre), the last column,
    # row 0 with the partner in row 1, the last row with the partner in the row above; (1, 0) tangents are vertical, so xr = qx
    kl = keylines(4)
    kl["pos"] = ((0.0, 10.0), (COLS - 1.0, 20.0), (40.0, 0.0), (40.0, ROWS - 1.0))
    ent = [(0, 10, -0.25, 10.0, 1.0, 0.0, 1.0), at(COLS - 6.0, 20.0), at(35.0, 1.0), at(35.0, ROWS - 2.0), at(COLS - 1.0, 21.0)]
    case("borders", kl, ent, [1, 1, 1, 1], [0, 1, 2, 3])
    case("borders_row_tol_0", kl, ent, [1, 1, 0, 0], [0, 1, -1, -1], row_tol=0)

    # a window clipped to nothing (every cell holds a keyline), and positions that are no position
    kl = keylines(6)
    kl["pos"] = ((2.0, 5.0), (NAN, 5.0), (5.0, np.inf), (-np.inf, NAN), (1e30, 5.0), (-0.75, 5.0))
    ent = [at(float(x), 5.0) for x in range(0, 40)]
    case("no_window", kl, ent, [0, 0, 0, 0, 0, 0], d_min=10.0, d_max=20.0)

    # d_min = 3: a keyline at column 2 has the one-cell window [0, 0], one at column 1 none; the partner's position lies left of its cell
    kl = keylines(2)
    kl["pos"] = ((2.0, 5.0), (1.0, 15.0))
    ent = [(0, 5, -1.5, 5.0, 1.0, 0.0, 1.0), (0, 15, -2.5, 15.0, 1.0, 0.0, 1.0)]
    case("one_cell", kl, ent, [1, 0], [0, -1], d_min=3.0, d_max=9.0)

    # d exactly d_min and d_max are candidates; one ulp outside and d = 0 are not
    kl = keylines(5)
    kl["pos"] = [(40.0, 3.0 * i + 2) for i in range(5)]
    ent = [at(37.0, 2.0), at(33.0, 5.0), at(up(37.0), 8.0), at(dn(33.0), 11.0), at(40.0, 14.0)]
    case("d_bounds", kl, ent, [1, 1, 0, 0, 0], [0, 1, -1, -1, -1], d_min=3.0, d_max=7.0, row_tol=0)
    case("d_zero", kl[4:], ent, [0], [-1], row_tol=0)

    # an innovation exactly at the gate: v = 0, s_m = 2.5 / 10, gate 2: in while e * e <= 0.25; d = 5: rho_m = 0.5
    kl = keylines(3, sigma=0.0)
    kl["pos"] = [(40.0, 3.0 * i + 2) for i in range(3)]
    kl["rho"] = (1.0, up(1.0), 0.25)
    ent = [at(35.0, 3.0 * i + 2) for i in range(3)]
    case("gate", kl, ent, [1, 2, 1], [0, -1, 2], sigma_px=2.5, gate_sigma=2.0, row_tol=0)

    # a spread of exactly ambig_px is one surface, one ulp more is two
    kl = keylines(2)
    kl["pos"] = ((40.0, 5.0), (40.0, 15.0))
    ent = [at(35.0, 5.0), at(33.0, 5.0), at(35.0, 15.0), at(dn(33.0), 15.0)]
    case("ambiguity", kl, ent, [1, 4], None, row_tol=0)

    # a score tie goes to the smaller j, whichever cell is met first; a better score beats a smaller j
    kl = keylines(2)
    kl["pos"] = ((40.0, 5.0), (40.0, 15.0))
    ent = [at(35.0, 5.0), at(34.0, 5.0), at(34.0, 15.0), at(35.0, 15.0), at(35.5, 16.0, 1.0, 0.0, 1.0)]
    ent[2] = at(34.0, 15.0, 1.0, 0.25, F32(1.0625) ** F32(0.5))
    case("tie", kl, ent, [1, 1], [0, 3])

    # both clamps (fm, baseline: fb = 0.1 and 10000), and a certain keyline
    kl = keylines(1)
    kl["pos"] = (40.0, 5.0)
    case("clamp_high", kl, [at(35.0, 5.0)], [33], [0], baseline=0.00125)
    case("clamp_low", kl, [at(35.0, 5.0)], [33], [0], baseline=125.0)
    kl = keylines(2, rho=0.5, sigma=0.0)
    kl["pos"] = ((40.0, 5.0), (40.0, 15.0))
    kl["rho"][1] = 0.6
    ent = [at(35.0, 5.0), at(35.0, 15.0)]
    case("sigma_zero", kl, ent, [1, 2], [0, -1], sigma_px=0.1, row_tol=0)
    case("sigma_zero_q_abs", kl, ent, [1, 1], [0, 1], sigma_px=0.1, row_tol=0, q_abs=1.0)

    # the right keyline's own tests: no norm, the angle, the norm ratio, its direction, NaN position; a mask word behind the table
    kl = keylines(7)
    kl["pos"] = [(40.0, 3.0 * i + 2) for i in range(7)]
    ent = [at(35.0, 2.0, 1.0, 0.0, 0.0), at(35.0, 5.0, 0.6, 0.8, 1.0), at(35.0, 8.0, 2.5, 0.0, 2.5), at(35.0, 11.0, 2.0, 0.0, 2.0),
           (35, 14, NAN, 14.0, 1.0, 0.0, 1.0), at(35.0, 17.0, -1.0, 0.0, 1.0)]
    kr, mask = plant(ROWS, COLS, ent)
    mask[20, 35] = 6  # behind the right table's end
    out.append(("right_tests", ROWS, COLS, FM, kl, kr, mask, dict(baseline=BASE, row_tol=0), [0, 0, 0, 1, 0, 0, 0], [-1, -1, -1, 3, -1, -1, -1]))

    # empty maps
    out.append(("empty_right", ROWS, COLS, FM, keylines(3), keylines(0), np.full((ROWS, COLS), -1, np.int32), dict(baseline=BASE), [0, 0, 0], None))
    case("empty_left", keylines(0), [at(35.0, 5.0)], [], [])

    # a 37x33 image: keylines in its corners and a partner for each inside a window that is clipped on two sides
    kl = keylines(4)
    kl["pos"] = ((36.0, 0.0), (36.0, 32.0), (3.0, 0.0), (3.0, 32.0))
    ent = [at(30.0, 1.0), at(30.0, 31.0), at(1.0, 0.0), at(0.0, 32.0)]
    case("37x33", kl, ent, [1, 1, 1, 1], [0, 1, 2, 3], rows=33, cols=37, d_max=20.0)
    return out


def random_right_map(rng, rows, cols, n):
    """n keylines in distinct cells, sub-pixel positions, gradients of every direction, a few without a norm"""
    cells = rng.choice(rows * cols, n, replace=False)
    kr = keylines(n)
    cy, cx = np.divmod(cells, cols)
    kr["pos"][:, 0] = (cx + rng.uniform(-0.5, 0.5, n)).astype(F32)
    kr["pos"][:, 1] = (cy + rng.uniform(-0.5, 0.5, n)).astype(F32)
    g = rng.normal(0, 5, (n, 2))
    g[:, 0] += np.where(rng.uniform(size=n) < 0.5, 6.0, 0.0)
    kr["gradient"] = g.astype(F32)
    kr["gradient_norm"] = np.sqrt((kr["gradient"].astype(np.float64) ** 2).sum(1)).astype(F32)
    kr["gradient_norm"][rng.uniform(size=n) < 0.02] = 0.0
    mask = np.full(rows * cols, -1, np.int32)
    mask[cells] = np.arange(n)
    return kr, mask.reshape(rows, cols)


def left_from_right(rng, kr, rows, cols, n, fb, d_hi=40.0):
    """n left keylines crafted from a right table: most are a right keyline moved by a disparity, with its gradient disturbed and a
    prior that agrees with the disparity, disagrees, or is fresh; the rest lie anywhere, some outside the image or without a
    direction."""
    kl = keylines(n)
    if n == 0:
        return kl
    if len(kr):
        src = rng.integers(0, len(kr), n)
        d = rng.uniform(0.0, d_hi, n)
        kl["pos"][:, 0] = (kr["pos"][src, 0] + d).astype(F32)
        kl["pos"][:, 1] = (kr["pos"][src, 1] + rng.choice([0.0, 0.0, 0.3, -0.4, 1.0, -1.0], n)).astype(F32)
        kl["gradient"] = (kr["gradient"][src] * rng.uniform(0.8, 1.25, (n, 1)) + rng.normal(0, 0.3, (n, 2))).astype(F32)
    else:
        d = rng.uniform(0.0, d_hi, n)
        kl["pos"] = rng.uniform(0, max(rows, cols), (n, 2)).astype(F32)
        kl["gradient"] = rng.normal(0, 5, (n, 2)).astype(F32)
    kl["gradient_norm"] = np.sqrt((kl["gradient"].astype(np.float64) ** 2).sum(1)).astype(F32)
    kind = rng.integers(0, 4, n)
    kl["rho"] = np.where(kind == 0, 1.0, np.where(kind == 1, d / fb, rng.uniform(0.001, 3.0, n))).astype(F32)
    kl["sigma_rho"] = np.where(kind == 0, 20.0, np.where(kind == 1, rng.uniform(0.0, 0.1, n), rng.uniform(0.0, 2.0, n))).astype(F32)
    wild = rng.uniform(size=n) < 0.1
    kl["pos"][wild] = rng.uniform(-3, max(rows, cols) + 3, (int(wild.sum()), 2)).astype(F32)
    kl["gradient_norm"][rng.uniform(size=n) < 0.02] = 0.0
    kl["matches"] = rng.integers(0, 9, n)
    return kl
