"""Cameras, frames and an independent statement for the lens front end (k_front_end_u8 and its _px / _b forms, hm::undistort_fixed_map,
orc_front_end_u8): what tests/test_lens_front_end.py holds the oracle and the host map function to on the CPU and
tests/test_lens_front_end_gpu.py holds the kernels to. A plain module: no test, no GPU, numpy alone.

A case is (cols, rows, fx, fy, cx, cy, D) with D = k1, k2, p1, p2, k3. The intrinsics are rounded to fp32 before anything is
computed from them, as the ABI takes them (K4, D5 are float arrays).

direct_map states cv::undistort's map as published, straight from the pixel indices in np.longdouble:
    x = (j - cx) / fx, y = (i - cy) / fy, r2 = x^2 + y^2, kr = 1 + ((k3 r2 + k2) r2 + k1) r2
    u = fx (x kr + 2 p1 x y + p2 (r2 + 2 x^2)) + cx,  v = fy (y kr + p1 (r2 + 2 y^2) + 2 p2 x y) + cy
with no stripes, no running sum of 1/fx and no shifted principal point, so it shares none of the structure of the two double
implementations. The map words are rint(32 u), rint(32 v), saturated to int (a NaN to INT_MIN). A double implementation can
only differ from them where 32 u lies within its own rounding error (about 1e-9 at these sizes) of a half-integer; the tests
assert that every camera here keeps 1e-6 away from one over its whole frame, and then compare without a tolerance."""
import functools

import numpy as np

LD = np.longdouble
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
EUROC_K = (458.654, 457.296, 367.215, 248.375)                      # the EuRoC camera's fx, fy, cx, cy at 752x480
EUROC_D = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0)
MIN_TIE = 1e-6         # of a 1/32 px unit: the condition on the inputs under which a map is compared word for word
MIN_PLANT = 1e-3       # of a 1/32 px unit: how far a planted pixel stays from any rounding boundary

# name: (cols, rows, fx, fy, cx, cy, D)
CAMERAS = {
    "euroc-quarter": (188, 120) + tuple(k / 4 for k in EUROC_K) + (EUROC_D,),                       # fx != fy, off-centre
    "pincushion-150-140": (200, 150, 150.0, 140.0, 101.3, 73.9, (0.6, -0.1, 1e-3, -2e-3, 0.05)),    # reads the border
    "corner-principal-point": (160, 120, 120.0, 118.0, 20.25, 120 - 19.25, (0.12, -0.02, 4e-3, -2e-3, 0.0)),
    "principal-point-outside": (131, 67, 90.0, 95.0, -29.5, 80.2, (-0.1, 0.01, 5e-4, 3e-4, 0.0)),
    "nearly-identity": (255, 255, 200.3, 199.1, 127.2, 126.6, (1e-7, 0.0, 0.0, 0.0, 0.0)),          # every pixel reads itself
    "tangential-only": (188, 120, 110.0, 112.0, 95.1, 58.7, (0.0, 0.0, 4e-3, -3e-3, 0.0)),
    # cy one fp32 step below the calibration's 248.375, at which one pixel of the frame comes within 5.6e-7 of a tie
    "euroc-full": (752, 480) + EUROC_K[:3] + (248.37498474121094, EUROC_D),
}
SMALL = tuple(n for n, c in CAMERAS.items() if c[0] <= 255 and c[1] <= 255)      # the ramp frames decode these
MAP_SIZES = ((37, 33), (131, 67), (188, 120), (255, 255))    # 37 * 33 = 1221 pixels: a partial last workgroup of 256
STRIPE_WIDTHS = (1365, 1366, 4096)                           # cv::undistort's stripes of 4096 / cols = 3, 2 and 1 rows
STRIPE_ROWS = 35       # the fewest rows a context takes (32 at least) that leave the last stripe of 3 and of 2 rows ragged


def f32_case(case):
    """the case as the ABI sees it: every intrinsic an fp32 value, held in longdouble"""
    cols, rows, fx, fy, cx, cy, D = case
    K = [LD(np.float32(v)) for v in (fx, fy, cx, cy)]
    return cols, rows, K[0], K[1], K[2], K[3], [LD(np.float32(d)) for d in D]


def K4(case):
    return tuple(float(np.float32(v)) for v in case[2:6])


def D5(case):
    return [float(np.float32(v)) for v in case[6]]


def at_size(case, cols, rows):
    """the camera seen at another image size: focal lengths and principal point scaled per axis, the coefficients kept"""
    c0, r0, fx, fy, cx, cy, D = case
    return (cols, rows, fx * cols / c0, fy * rows / r0, cx * cols / c0, cy * rows / r0, D)


def stripe_case(cols, rows=STRIPE_ROWS):
    """cols x rows with fx != fy and cy off the centre: 4096 / cols rows per stripe of cv::undistort"""
    return (cols, rows, 0.61 * cols, 0.57 * cols, 0.47 * cols + 0.3, 0.31 * rows + 0.3, (-0.28, 0.07, 2e-3, -1e-3, 0.01))


def _tie(w):
    """distance of 32 u to the nearest point where its rounded word changes: a half-integer, or the edge of int's range"""
    with np.errstate(invalid="ignore"):
        d = np.abs(w - np.floor(w) - LD(0.5))
        d = np.where(w >= LD(INT_MAX), np.abs(w - (LD(INT_MAX) + LD(0.5))), d)
        d = np.where(w <= LD(INT_MIN), np.abs(w - (LD(INT_MIN) - LD(0.5))), d)
    return np.where(np.isnan(w), LD(np.inf), d)


@functools.lru_cache(maxsize=None)
def direct_map(case):
    """(32 u, 32 v, tie distance of 32 u, tie distance of 32 v), each [rows, cols] in np.longdouble; computed once per case
    (a case is a tuple of numbers and one tuple of coefficients) and not to be written to"""
    cols, rows, fx, fy, cx, cy, (k1, k2, p1, p2, k3) = f32_case(case)
    j, i = np.meshgrid(np.arange(cols).astype(LD), np.arange(rows).astype(LD))
    with np.errstate(all="ignore"):
        x, y = (j - cx) / fx, (i - cy) / fy
        r2 = x * x + y * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        u = fx * (x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)) + cx
        v = fy * (y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y) + cy
        wu, wv = u * 32, v * 32
    return wu, wv, _tie(wu), _tie(wv)


def _word(w):
    with np.errstate(invalid="ignore"):
        r = np.clip(np.rint(w), LD(INT_MIN), LD(INT_MAX))
    return np.where(np.isnan(w), LD(INT_MIN), r).astype(np.int64)


def map_words(case):
    """(iu, iv) int64 [rows, cols]: rint of direct_map, saturated to int, a NaN to INT_MIN"""
    wu, wv, _, _ = direct_map(case)
    return _word(wu), _word(wv)


def min_tie(case):
    _, _, du, dv = direct_map(case)
    return float(min(du.min(), dv.min()))


def inside(iu, iv, cols, rows):
    """where all four taps of a pixel lie inside the image"""
    sx, sy = iu >> 5, iv >> 5
    return (sx >= 0) & (sx + 1 < cols) & (sy >= 0) & (sy + 1 < rows)


def remap(iu, iv, frame):
    """convertTo(CV_32F, 3.0) + remap(INTER_LINEAR, BORDER_CONSTANT 0) through the map words: 3 * sum of tap * weight with the
    weights (32 - a)(32 - b) / 1024. Taps are below 2^8, weights' numerators at most 2^10, so the integer sum is exact and its
    fp32 value is the one any order of exact fp32 products and sums gives."""
    rows, cols = frame.shape
    sx, sy, ax, ay = iu >> 5, iv >> 5, iu & 31, iv & 31
    src = frame.astype(np.int64)

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < cols) & (yy >= 0) & (yy < rows)
        return np.where(ok, src[np.clip(yy, 0, rows - 1), np.clip(xx, 0, cols - 1)], 0)

    s = ((32 - ay) * (32 - ax) * tap(sy, sx) + (32 - ay) * ax * tap(sy, sx + 1) + ay * (32 - ax) * tap(sy + 1, sx)
         + ay * ax * tap(sy + 1, sx + 1))
    out = (3 * s).astype(np.float64) / 1024.0
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)
    return out.astype(np.float32)


def ramp_frames(cols, rows):
    """(pixel = column index, pixel = row index) as u8 frames, cols, rows <= 255. Where all four taps are inside,
    front end(column ramp) = 3 (sx + ax / 32) = 3 iu / 32 exactly, and the row ramp gives 3 iv / 32."""
    assert cols <= 255 and rows <= 255, (cols, rows)
    j, i = np.meshgrid(np.arange(cols), np.arange(rows))
    return j.astype(np.uint8), i.astype(np.uint8)


def decode_ramp(out):
    """the map word a ramp frame's front end output holds: out * 32 / 3, which has to be an integer"""
    w = out.astype(np.float64) * 32.0 / 3.0
    r = np.rint(w)
    return r.astype(np.int64), (r * 3.0 == out.astype(np.float64) * 32.0)


def weave_frame(cols, rows):
    """pixel = (7 col + 13 row) & 255: any two of the 3 x 3 pixels around a tap differ, at any width"""
    j, i = np.meshgrid(np.arange(cols), np.arange(rows))
    return ((7 * j + 13 * i) & 255).astype(np.uint8)


# ---- planted pixels ---------------------------------------------------------------------------------------------------------
# One camera per planted pixel, 96 x 64 unless another size is asked for, with fx = fy = 40 and D = (k1, 0, 0, 0, 0). A pixel of
# the row i = cy has y = 0, so v = cy exactly and u = fx x (1 + k1 x^2) + cx with x = (j - cx) / fx; k1 = ((u - cx) / (fx x) - 1)
# / x^2 puts it at any u. A pixel of the column j = cx is placed at any v the same way. k1 is then an fp32 value (the nearest
# few are tried, the best kept), and the module asserts in longdouble where the pixel really lands.
# Along x the principal point is (cols / 2 - 0.5, rows / 2) and the planted pixel (rows / 2, cols - 6): at 96 x 64 that is
# cx = 47.5, cy = 32, pixel (row 32, col 90). Along y it is (cols / 2, rows / 2 - 0.5) and (rows - 4, cols / 2).
P_COLS, P_ROWS, P_F = 96, 64, 40.0
# name: (axis, the coordinate the pixel is sent to at cols x rows, what it reads)
PLANTS = {
    "sx=-1": ("x", lambda cols, rows: -1 + 16 / 32, "right taps only"),
    "sx=cols-1": ("x", lambda cols, rows: cols - 1 + 8 / 32, "left taps only"),
    "sx=-2": ("x", lambda cols, rows: -2 + 16 / 32, "border"),
    "sx=cols": ("x", lambda cols, rows: cols + 8 / 32, "border"),
    "sy=-1": ("y", lambda cols, rows: -1 + 24 / 32, "lower taps only"),
    "sy=rows-1": ("y", lambda cols, rows: rows - 1 + 8 / 32, "upper taps only"),
    "fraction-0": ("x", lambda cols, rows: 10.0, "one tap"),
    "fraction-31/32": ("x", lambda cols, rows: 10 + 31 / 32, "two taps"),
    "just-above-32767": ("x", lambda cols, rows: 32768 + 8 / 32, "border"),
    "just-below--32768": ("x", lambda cols, rows: -32769 + 8 / 32, "border"),
    "wrap-65536+10": ("x", lambda cols, rows: 65536 + 10 + 8 / 32, "border"),        # a wrapping (short) reads column 10
    "wrap--65536+10": ("x", lambda cols, rows: -65536 + 10 + 8 / 32, "border"),
    "wrap-y-65536+10": ("y", lambda cols, rows: 65536 + 10 + 8 / 32, "border"),
    "beyond-2^31": ("x", lambda cols, rows: 1.5 * 2 ** 31 / 32, "border"),           # 32 u = 1.5 * 2^31: saturates to INT_MAX
    "beyond--2^31": ("x", lambda cols, rows: -1.5 * 2 ** 31 / 32, "border"),
}


@functools.lru_cache(maxsize=None)
def planted(name, cols=P_COLS, rows=P_ROWS):
    """(case, (row, col), (iu, iv)): the camera, the planted pixel and the map words it has there"""
    axis, target, _ = PLANTS[name]
    target = target(cols, rows)
    if axis == "x":
        cx, cy, row, col = cols / 2 - 0.5, float(rows // 2), rows // 2, cols - 6
        n, c0 = (LD(col) - LD(cx)) / LD(P_F), LD(cx)
    else:
        cx, cy, row, col = float(cols // 2), rows / 2 - 0.5, rows - 4, cols // 2
        n, c0 = (LD(row) - LD(cy)) / LD(P_F), LD(cy)
    k1 = np.float32(float(((LD(target) - c0) / (LD(P_F) * n) - 1) / (n * n)))
    want = LD(target) * 32
    best = None
    for step in range(-3, 4):
        k = k1
        for _ in range(abs(step)):
            k = np.nextafter(k, np.float32(np.inf if step > 0 else -np.inf))
        w = (LD(P_F) * n * (1 + LD(k) * n * n) + c0) * 32
        if best is None or abs(w - want) < best[0]:
            best = (abs(w - want), k)
    case = (cols, rows, P_F, P_F, cx, cy, (float(best[1]), 0.0, 0.0, 0.0, 0.0))
    wu, wv, du, dv = direct_map(case)
    iu, iv = map_words(case)
    w_along, d_along, w_across = (wu, du, wv) if axis == "x" else (wv, dv, wu)
    # where it is meant to be: the word of the target along the axis, the principal point's own coordinate across it
    sat = int(np.clip(np.rint(want), LD(INT_MIN), LD(INT_MAX)))
    got = int((iu if axis == "x" else iv)[row, col])
    assert got == sat, (name, got, sat)
    assert d_along[row, col] >= MIN_PLANT, (name, float(d_along[row, col]))
    assert w_across[row, col] == (LD(cy) if axis == "x" else LD(cx)) * 32, name
    if abs(target) * 32 >= 2 ** 31:
        assert abs(w_along[row, col]) > LD(2) ** 31, name
    return case, (row, col), (int(iu[row, col]), int(iv[row, col]))


def planted_value(name, frame):
    """what the planted pixel reads from a u8 frame, by hand from the words it was planted at: taps and weights written out"""
    rows, cols = frame.shape
    case, (row, col), (iu, iv) = planted(name, cols, rows)
    sx, sy, ax, ay = iu >> 5, iv >> 5, iu & 31, iv & 31
    total = 0
    for dy, wy in ((0, 32 - ay), (1, ay)):
        for dx, wx in ((0, 32 - ax), (1, ax)):
            if 0 <= sx + dx < cols and 0 <= sy + dy < rows:
                total += wy * wx * int(frame[sy + dy, sx + dx])
    return np.float32(3 * total / 1024.0)
