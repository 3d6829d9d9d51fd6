"""GPU parity of keyline detection away from the defaults and on crafted images: the four gates of the candidate test
(edge_detector.cpp:73-107) swept and put exactly on equality, the threshold servo into both clamps and with the clamps inverted,
joinEdges on images whose edges run along the rim of the plane-fit interior and fork, and the batch spelling of the candidate
test (keyline_flag_body behind k_dog_mag_b) next to the single-stream one (keyline_flag_ii_body).

Every comparison is bit for bit against the CPU oracle; this file adds no tolerance. Expectations come from the oracle or from
plain numpy, never from the library. A case that claims to reach something asserts that on the oracle alone, before the library
is looked at; the oracle's own figures, as measured when the file was written, stand in the docstrings.

No case constructs a configuration rebvio_hip_create refuses (tests/test_abi.py).
"""
import numpy as np
import pytest

from conftest import params_for
from support import B  # noqa: F401
from support import (F32, assert_keylines_equal, assert_map, assert_pipeline_bit_identical, masked_map, record_words, run_stream,
                     set_forms)

pytestmark = pytest.mark.gpu

# the base case: the servo off, so that the gates see exactly the configured threshold
BASE = dict(keylines_ref=1500, keylines_max=6000, gain=0.0)


def _bits(x):
    return np.asarray(x, F32).reshape(-1).view(np.uint32)


def assert_detect_equal(orc, ctx, om, gm, what):
    """the "detect comparison": map size, every keyline field, the dense mask, the map's threshold and the detector's state"""
    H, W = orc.rows, orc.cols
    assert om.size() == gm.size(), (what, om.size(), gm.size())
    assert_keylines_equal(om.keylines(), gm.keylines(), what=what)
    mo, mg = om.mask(H, W), gm.mask()
    assert np.array_equal(mo, mg), (what, "mask", np.argwhere(mo != mg)[:4].tolist())
    assert np.array_equal(_bits(om.threshold), _bits(gm.threshold)), (what, om.threshold, gm.threshold)
    thr, auto, cnt = ctx.detector_state()
    assert np.array_equal(_bits(thr), _bits(orc.threshold)), (what, thr, orc.threshold)
    assert np.array_equal(_bits(auto), _bits(orc.auto_threshold)), (what, auto, orc.auto_threshold)
    assert cnt == om.size(), (what, cnt, om.size())


def detect_both(orc_mod, B, cam_or_size, frames, kw, what, mask=None):
    """frames through a fresh oracle and a fresh context, a detect comparison on every frame; returns the oracle's counts.
    mask: a static detection mask for the library; the expectation is then the oracle's unmasked map with the masked pixels
    dropped (support.masked_map; gain must be 0 and nothing may be truncated)."""
    if isinstance(cam_or_size, tuple):
        H, W = cam_or_size
        orc = orc_mod.Oracle(orc_mod.default_params(H, W, **kw))
        ctx = B.Context(B.default_params(H, W, **kw))
    else:
        H, W = cam_or_size.height, cam_or_size.width
        orc = orc_mod.Oracle(params_for(orc_mod, cam_or_size, **kw))
        ctx = B.Context(params_for(B, cam_or_size, **kw))
    if mask is not None:
        assert kw["gain"] == 0.0
        ctx.set_detection_mask(mask)
    counts = []
    auto = F32(ctx.p.threshold)
    for k, f in enumerate(frames):
        om, gm = orc.detect_u8(f, k * 50000), ctx.detect_u8(f, k * 50000)
        if mask is None:
            assert_detect_equal(orc, ctx, om, gm, f"{what} frame {k}")
            counts.append(om.size())
        else:
            want = masked_map(om, H, W, mask, kw["keylines_max"], auto)
            assert om.size() < kw["keylines_max"] and 0 < len(want[0]) < om.size(), (what, om.size(), len(want[0]))
            assert_map(want, gm, f"{what} frame {k}, masked")
            thr, a_dev, cnt = ctx.detector_state()
            assert cnt == len(want[0]) and np.array_equal(_bits(a_dev), _bits(want[2])) and np.array_equal(_bits(thr), _bits(orc.threshold))
            auto = want[2]
            counts.append(len(want[0]))
        gm.release()
    ctx.close()
    return counts


_oracle_counts = {}


def oracle_count(orc_mod, cam, frame, **kw):
    """keylines the oracle finds in one frame (first frame of a context) at BASE + kw; once per configuration"""
    key = tuple(sorted((k, float(v)) for k, v in kw.items()))
    if key not in _oracle_counts:
        _oracle_counts[key] = orc_mod.Oracle(params_for(orc_mod, cam, **dict(BASE, **kw))).detect_u8(frame, 0).size()
    return _oracle_counts[key]


# ---- a. gate sweeps ------------------------------------------------------------------------------------------------------
# 25 x pos_neg_threshold lies on (1, 3, 5, 7, 9, 15, 25) or next to (0) the odd integers |pn| takes
SWEEPS = {
    "pos_neg_threshold": [0.0, 0.04, 0.12, 0.2, 0.28, 0.36, 0.6, 1.0],
    "dog_threshold": [0.01, 0.05, 0.3, 1.0, 3.0],
    "threshold": [0.001, 0.005, 0.05, 0.2],
}
# pairs of neighbours documented as saturated: the gate no longer rejects anything there
SATURATED = {("pos_neg_threshold", 0.6, 1.0)}
COMBINED = dict(pos_neg_threshold=0.2, dog_threshold=0.3, threshold=0.005)
# the oracle's keyline counts on frame 0 of the 192x144 stream, as the docstrings quote them: asserted, so that they cannot go stale
SWEEP_COUNTS = {
    "pos_neg_threshold": [0, 607, 1163, 1733, 2024, 2103, 2122, 2122],
    "dog_threshold": [2113, 2112, 1684, 157, 0],
    "threshold": [3162, 2451, 644, 0],
}


def sweep_counts(orc_mod, small_stream):
    frames, cam = small_stream
    return {name: [oracle_count(orc_mod, cam, frames[0], **{name: v}) for v in vals] for name, vals in SWEEPS.items()}


def assert_sweep_moves(orc_mod, small_stream, name):
    """Precondition, on the oracle alone: every value of the sweep changes the keyline count from its neighbour's, except the
    pairs listed as saturated, which must be equal."""
    counts = sweep_counts(orc_mod, small_stream)[name]
    vals = SWEEPS[name]
    for (a, na), (b, nb) in zip(zip(vals, counts), zip(vals[1:], counts[1:])):
        if (name, a, b) in SATURATED:
            assert na == nb, (name, a, b, na, nb)
        else:
            assert na != nb, (name, a, b, na, nb)
    assert counts == SWEEP_COUNTS[name], (name, counts)
    return counts


@pytest.mark.parametrize("name,value", [(n, v) for n, vals in SWEEPS.items() for v in vals],
                         ids=[f"{n}={v}" for n, vals in SWEEPS.items() for v in vals])
def test_gate_sweep(orc_mod, B, small_stream, name, value):
    """One gate parameter off its default on the 192x144 stream, servo off. The oracle's keyline counts on frame 0 (default: 2103):
      pos_neg_threshold 0 / 0.04 / 0.12 / 0.2 / 0.28 / 0.36 / 0.6 / 1.0: 0, 607, 1163, 1733, 2024, 2103, 2122, 2122
        (0.6 against 1.0 is saturated: 25 x 0.6 = 15 is already above every |pn| that reaches the gate here; asserted as such)
      dog_threshold 0.01 / 0.05 / 0.3 / 1.0 / 3.0: 2113, 2112, 1684, 157, 0
      threshold 0.001 / 0.005 / 0.05 / 0.2: 3162, 2451, 644, 0
    Two frames each, so that an empty first map is followed by another detect."""
    frames, cam = small_stream
    counts = assert_sweep_moves(orc_mod, small_stream, name)
    got = detect_both(orc_mod, B, cam, frames[:2], dict(BASE, **{name: value}), f"{name}={value}")
    assert got[0] == counts[SWEEPS[name].index(value)]


def test_gate_sweep_combined(orc_mod, B, small_stream):
    """All three gate parameters moved at once."""
    frames, cam = small_stream
    n = oracle_count(orc_mod, cam, frames[0], **COMBINED)
    singles = [oracle_count(orc_mod, cam, frames[0], **{k: v}) for k, v in COMBINED.items()]
    assert 0 < n and all(n != s for s in singles), (n, singles)
    detect_both(orc_mod, B, cam, frames[:3], dict(BASE, **COMBINED), "combined")


@pytest.mark.parametrize("kw", [dict(pos_neg_threshold=0.12), dict(dog_threshold=0.3), dict(threshold=0.005), COMBINED],
                         ids=["pos_neg_threshold=0.12", "dog_threshold=0.3", "threshold=0.005", "combined"])
def test_gate_sweep_under_a_static_mask(orc_mod, B, small_stream, kw):
    """One value of each sweep through the masked instance of the kernel: a static mask that keeps the left half of the frame
    and every third row of the right half."""
    frames, cam = small_stream
    keep = np.zeros((cam.height, cam.width), np.uint8)
    keep[:, :cam.width // 2] = 1
    keep[::3, cam.width // 2:] = 7
    detect_both(orc_mod, B, cam, frames[:2], dict(BASE, **kw), f"masked {kw}", mask=keep)


# ---- b. the gates exactly at equality -----------------------------------------------------------------------------------------
N_EQ = 8


def reachable(values, to_bound, guess):
    """For each fp32 value v: the largest fp32 t within +-3 ulp of guess(v) whose bound to_bound(t) - evaluated in fp32 as the
    kernels spell it - equals v while that of the next fp32 above t exceeds it. Returns [(v, t)] for the values that have one."""
    out = []
    for v in values:
        t0 = F32(guess(v))
        cand = [t0]
        for _ in range(3):
            cand.append(np.nextafter(cand[-1], F32(np.inf)))
        lo = t0
        for _ in range(3):
            lo = np.nextafter(lo, F32(0))
            cand.append(lo)
        hits = [t for t in cand if to_bound(t) == v and to_bound(np.nextafter(t, F32(np.inf))) > v]
        if hits:
            out.append((F32(v), max(hits)))
    return out


def mag_bound(t):
    a = F32(F32(t) * F32(765))
    return F32(a * a)          # mag_threshold = (thr * 765) * (thr * 765)


def grad_bound(d, thr=F32(0.01)):
    a = F32(F32(F32(thr) * F32(765)) * F32(d))
    return F32(a * a)          # gradient_threshold_squared = (thr * 765 * dog_threshold) * (thr * 765 * dog_threshold)


def spread(items, n):
    return [items[i] for i in np.linspace(0, len(items) - 1, n).round().astype(int)]


_equality = {}


def equality_cases(orc_mod, small_stream, gate):
    """N_EQ (value, parameter) pairs for the gate, spread over the range, chosen on the oracle alone: the value is reachable
    as the gate's bound and the oracle finds fewer keylines with the parameter one ulp above the value than with it on the value."""
    if gate in _equality:
        return _equality[gate]
    frames, cam = small_stream
    H, W = cam.height, cam.width
    if gate == "magnitude":
        # squared gradient magnitudes (scale_space.cpp:221-232) of the interior pixels that pass the other gates at a low
        # threshold: elsewhere the magnitude gate decides nothing
        orc = orc_mod.Oracle(params_for(orc_mod, cam, **dict(BASE, threshold=0.001)))
        mag = orc.scale_space(frames[0].astype(F32) * F32(3.0))["mag"]
        mag = mag[orc.detect_u8(frames[0], 0).mask(H, W) >= 0]
        vals = np.unique(mag[(mag > 30) & (mag < 300)])
        reach = reachable(vals, mag_bound, lambda v: np.sqrt(np.float64(v)) / 765.0)
        name = "threshold"
    else:
        # squared plane-fit gradients of the keylines at the default threshold, above the default bound
        kl = orc_mod.Oracle(params_for(orc_mod, cam, **BASE)).detect_u8(frames[0], 0).keylines()
        gx, gy = kl["gradient"][:, 0], kl["gradient"][:, 1]
        vals = np.unique(F32(gx * gx) + F32(gy * gy))
        t765 = np.float64(F32(F32(0.01) * F32(765)))
        reach = reachable(vals, grad_bound, lambda v: np.sqrt(np.float64(v)) / t765)
        reach = [(v, d) for v, d in reach if d < 1.0]   # (beyond dog_threshold = 1 nearly nothing is left to count)
        name = "dog_threshold"
    assert len(reach) >= N_EQ, (gate, len(vals), len(reach))
    biting = []
    for v, t in spread(reach, min(len(reach), 5 * N_EQ)):
        on = oracle_count(orc_mod, cam, frames[0], **{name: float(t)})
        above = oracle_count(orc_mod, cam, frames[0], **{name: float(np.nextafter(t, F32(np.inf)))})
        if on > above:
            biting.append((v, t, on, above))
    assert len(biting) >= N_EQ, (gate, len(reach), len(biting))
    _equality[gate] = (name, spread(biting, N_EQ), len(vals), len(reach))
    return _equality[gate]


@pytest.mark.parametrize("k", range(N_EQ))
@pytest.mark.parametrize("gate", ["magnitude", "gradient"])
def test_gate_at_equality(orc_mod, B, small_stream, gate, k):
    """The gates are !(x < bound): a value equal to the bound passes, with the bound one ulp higher it fails.
    magnitude: bound (threshold * 765)^2 put on a squared gradient magnitude of the interior (the oracle's scale space), through
    a threshold found within +-3 ulp of sqrt(v) / 765; gradient: bound ((0.01 * 765) * dog_threshold)^2 put on gx^2 + gy^2 of an
    oracle keyline, through a dog_threshold found the same way. Measured on the oracle: 486 distinct magnitudes in (30, 300) at
    pixels that pass the other gates, 217 of them reachable; 2103 distinct keyline gradients, 939 reachable with dog_threshold
    < 1. Eight per gate, spread over the range, each with the parameter on the value, one ulp below and one ulp above; the
    oracle finds more keylines on the value than above it - those that sit on the bound, one in each case measured (that is how
    the eight are chosen, from up to forty candidates)."""
    frames, cam = small_stream
    name, cases, _, _ = equality_cases(orc_mod, small_stream, gate)
    v, t, on, above = cases[k]
    assert on > above and (mag_bound(t) if gate == "magnitude" else grad_bound(t)) == v
    for what, p in (("on", t), ("below", np.nextafter(t, F32(0))), ("above", np.nextafter(t, F32(np.inf)))):
        got = detect_both(orc_mod, B, cam, frames[:1], dict(BASE, **{name: float(p)}), f"{gate} gate, {name} {what} {v!r}")
        if what != "below":
            assert got[0] == (on if what == "on" else above)


# ---- c. the threshold servo -------------------------------------------------------------------------------------------
SERVO = {
    "swing": dict(gain=5e-5, keylines_ref=1500),
    "pinned-low": dict(gain=5e-5, keylines_ref=4000),
    "climb": dict(gain=3e-6, min_threshold=0.012, max_threshold=0.02),
    "bang-bang": dict(gain=1e-3, keylines_ref=2000),
    "inverted": dict(gain=2e-6, min_threshold=0.03, max_threshold=0.02),
}
SERVO_FRAMES = 8


def servo_kw(name):
    return dict(dict(keylines_ref=1500, keylines_max=6000), **SERVO[name])


_servo_runs = {}


def servo_oracle(orc_mod, small_stream, name):
    """(thresholds the gates saw, keyline counts, final (threshold, auto threshold, count)) of the oracle over the eight frames"""
    if name not in _servo_runs:
        frames, cam = small_stream
        orc = orc_mod.Oracle(params_for(orc_mod, cam, **servo_kw(name)))
        thr, cnt = [], []
        for k in range(SERVO_FRAMES):
            m = orc.detect_u8(frames[k], k * 50000)
            thr.append(F32(orc.threshold))
            cnt.append(m.size())
        _servo_runs[name] = (thr, cnt, (F32(orc.threshold), F32(orc.auto_threshold), cnt[-1]))
    return _servo_runs[name]


def assert_servo_property(orc_mod, small_stream, name):
    """What each configuration is there for, asserted on the oracle alone."""
    thr, cnt, _ = servo_oracle(orc_mod, small_stream, name)
    lo, hi = F32(0.005), F32(0.5)
    if name == "swing":          # between the lower clamp, which it meets, and about 0.05
        assert min(thr) == lo and F32(0.04) < max(thr) < F32(0.06) and len(set(thr)) == SERVO_FRAMES, thr
    elif name == "pinned-low":
        assert all(t == lo for t in thr), thr
    elif name == "climb":        # from the lower clamp towards the upper
        assert thr[0] == F32(0.012) and all(a <= b for a, b in zip(thr, thr[1:])) and F32(0.012) < thr[-1] <= F32(0.02), thr
    elif name == "bang-bang":    # full maps at the lower clamp alternate with empty ones far above, the last on the upper clamp
        assert thr[0::2] == [lo] * 4 and all(t >= F32(0.45) for t in thr[1::2]) and thr[-1] == hi, thr
        assert all(c > 2000 for c in cnt[0::2]) and all(c == 0 for c in cnt[1::2]), cnt
    else:                        # inverted clamps: the order of the two comparisons decides
        assert thr[0] == F32(0.03) and thr[1] == F32(0.02) and set(thr) == {F32(0.03), F32(0.02)}, thr


@pytest.mark.parametrize("name", list(SERVO))
def test_servo_detect(orc_mod, B, small_stream, name):
    """Eight frames through detect_u8 with the servo on. The oracle's thresholds (counts), as measured:
      swing      0.005 (the lower clamp; 2451), 0.0525 (562), 0.0056, 0.0482, 0.0068, 0.0413, 0.0131, 0.0362
      pinned-low 0.005 on every frame (2451 to 2528 keylines of the 4000 asked for)
      climb      0.012 (the lower clamp), 0.0136, 0.0149, ... 0.0198, towards the upper clamp 0.02
      bang-bang  0.005 (about 2450 keylines) / 0.456, 0.469, 0.473 (0 keylines) in turn, ending on the upper clamp 0.5: the auto
                 threshold is carried across empty maps
      inverted   0.03, then 0.02 on every frame: min_threshold > max_threshold, the order of the two comparisons decides"""
    frames, cam = small_stream
    assert_servo_property(orc_mod, small_stream, name)
    got = detect_both(orc_mod, B, cam, frames[:SERVO_FRAMES], servo_kw(name), f"servo {name}")
    assert got == servo_oracle(orc_mod, small_stream, name)[1]


@pytest.mark.parametrize("name", ["swing", "climb"])
def test_servo_whole_pipeline(orc_mod, B, small_stream, name):
    """The per-pair API and the streaming driver, where the servo reads the previous frame's count on the device several frames
    ahead of the tracker: every word of every pair record, against the oracle with its sums in the kernels' order."""
    frames, cam = small_stream
    assert_servo_property(orc_mod, small_stream, name)
    kw = dict(servo_kw(name), global_min_matches_threshold=1)
    assert_pipeline_bit_identical(orc_mod, B, frames, cam, list(range(SERVO_FRAMES)), kw, 300, f"servo {name}")


@pytest.mark.parametrize("name", ["pinned-low", "bang-bang", "inverted"])
def test_servo_streaming_counts(orc_mod, B, small_stream, name):
    """The streaming driver on the configurations whose pairs are meant to fail: the keyline count that comes with every record
    and the detector's state after the flush."""
    frames, cam = small_stream
    assert_servo_property(orc_mod, small_stream, name)
    _, cnt, (thr, auto, last) = servo_oracle(orc_mod, small_stream, name)
    ctx = B.Context(params_for(B, cam, **servo_kw(name)))
    dev = ctx.upload_frames(frames[:SERVO_FRAMES])
    recs = run_stream(ctx, dev, range(SERVO_FRAMES), cam.width * cam.height)
    state = ctx.detector_state()
    ctx.close()
    assert [n for _, n in recs] == cnt[1:], (name, [n for _, n in recs], cnt)
    assert np.array_equal(_bits(state[0]), _bits(thr)) and np.array_equal(_bits(state[1]), _bits(auto)) and state[2] == last, (state, thr, auto, last)


# ---- d. crafted images ---------------------------------------------------------------------------------------------------
SIZES = [(131, 67), (100, 37), (192, 144)]   # (width, height): 131 is no multiple of 4, 67 / 37 none of 16
KW_IMG = dict(gain=0.0, keylines_ref=12000, keylines_max=20000)


def checkerboard(W, H):
    y, x = np.mgrid[0:H, 0:W]
    return np.where(((y + 5) // 8 + (x + 5) // 8) % 2 == 1, 220, 20).astype(np.uint8)


def star(W, H):
    """16 sectors about the centre: edges of every orientation meet in one point and leave through all four borders"""
    y, x = np.mgrid[0:H, 0:W]
    s = np.sin(8.0 * np.arctan2(y - (H - 1) / 2.0, x - (W - 1) / 2.0))
    return np.where(s > 0, 220, 20).astype(np.uint8)


def inset(W, H, k):
    img = np.full((H, W), 20, np.uint8)
    img[k:H - k, k:W - k] = 220
    return img


def bar(W, H):
    img = np.zeros((H, W), np.uint8)
    img[:, W // 3:W // 3 + 9] = 255
    return img


IMAGES = {"checkerboard": checkerboard, "star": star, "inset1": lambda W, H: inset(W, H, 1), "inset2": lambda W, H: inset(W, H, 2),
          "inset3": lambda W, H: inset(W, H, 3), "bar": bar}


def two_predecessors(kl):
    """keylines that two others name as their successor: joinEdges' "last writer of id_prev wins" """
    nxt = kl["id_next"][kl["id_next"] >= 0]
    return int((np.bincount(nxt, minlength=1) >= 2).sum())


def rim_counts(dense):
    """keylines on the four outermost lines of the plane-fit interior: row 2, row R-3, column 2, column C-3"""
    return [int((d >= 0).sum()) for d in (dense[2], dense[-3], dense[:, 2], dense[:, -3])]


def assert_image_preconditions(name, om, H, W):
    kl, dense = om.keylines(), om.mask(H, W)
    assert (dense[:2] < 0).all() and (dense[-2:] < 0).all() and (dense[:, :2] < 0).all() and (dense[:, -2:] < 0).all(), name
    if name.startswith("inset"):
        # a closed contour (every keyline has a successor) one to three pixels inside the rim on all four sides: the zero crossing
        # of the DoG moves inwards next to the border, where the box sums are cut off
        ys, xs = np.nonzero(dense >= 0)
        assert len(kl) > 200 and ys.min() <= 4 and ys.max() >= H - 5 and xs.min() <= 4 and xs.max() >= W - 5, (name, len(kl))
        return
    assert (kl["id_next"] < 0).any(), name
    if name in ("checkerboard", "star"):
        assert min(rim_counts(dense)) >= 1, (name, rim_counts(dense))
    if name == "checkerboard":
        assert two_predecessors(kl) >= 50, (name, two_predecessors(kl))


def assert_field_equal(orc, om, gm, what):
    orc.build_distance_field(om)
    ido, dso = orc.distance_field()
    idg, dsg = gm.distance_field()
    assert np.array_equal(ido, idg), (what, "field ids", (ido != idg).sum(), np.argwhere(ido != idg)[:3].tolist())
    sel = ido >= 0
    assert np.array_equal(dso[sel], dsg[sel]), (what, "field distances")


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("name", list(IMAGES))
def test_crafted_image(orc_mod, B, name, size):
    """Detection and the distance field of the map on images made for joinEdges and the rim of the interior. On the oracle,
    keylines / with two predecessors / without a successor / on row 2, row R-3, column 2, column C-3:
      checkerboard 131x67: 3106 / 217 / 24 / 35, 29, 19, 13;  100x37: 1096 / 78;  192x144: 11100 / 824
      star 131x67: 821 / 4 / 9 / 8, 8, 4, 4;  100x37: 448 / 3 / 13;  192x144: 1829 / 28 / 11
      inset 1, 2, 3 (238 to 667 keylines): closed contours one to three pixels inside the rim, every keyline with a successor
      bar (66 to 280 keylines): two straight chains that end on rows 2 and R-3
    and nothing in rows and columns 0-1, R-2, R-1, C-2, C-1 (asserted for every image)."""
    W, H = size
    img = IMAGES[name](W, H)
    orc = orc_mod.Oracle(orc_mod.default_params(H, W, **KW_IMG))
    ctx = B.Context(B.default_params(H, W, **KW_IMG))
    for k in range(2):   # (twice: the second map reuses what the first left in the detector)
        om = orc.detect_u8(img, k * 50000)
        if k == 0:
            assert_image_preconditions(name, om, H, W)
        gm = ctx.detect_u8(img, k * 50000)
        assert_detect_equal(orc, ctx, om, gm, f"{name} {W}x{H} frame {k}")
        if k == 0:
            gm.release()
    assert_field_equal(orc, om, gm, f"{name} {W}x{H}")
    gm.release()
    ctx.close()


@pytest.mark.parametrize("kmax", [4000, 4096])
def test_checkerboard_truncated_mid_frame(orc_mod, B, kmax):
    """keylines_max cuts the 192x144 checkerboard (11100 candidates) off in the middle of a row: the mask behind the cut is cleared
    before joinEdges probes it, so a keyline whose successor was cut (one at 4096) ends its chain."""
    W, H = 192, 144
    img = checkerboard(W, H)
    kw = dict(KW_IMG, keylines_max=kmax, keylines_ref=3000)
    orc = orc_mod.Oracle(orc_mod.default_params(H, W, **kw))
    ctx = B.Context(B.default_params(H, W, **kw))
    om = orc.detect_u8(img, 0)
    kl = om.keylines()
    full = orc_mod.Oracle(orc_mod.default_params(H, W, **KW_IMG)).detect_u8(img, 0)
    dense, dense_full = om.mask(H, W), full.mask(H, W)
    r = int(np.flatnonzero((dense >= 0).any(1)).max())   # the row the cut falls into: row 52 (22 of 46 kept) / 54 (27 of 45)
    assert len(kl) == kmax < full.size() and two_predecessors(kl) >= 50, (len(kl), full.size())
    assert 0 < (dense[r] >= 0).sum() < (dense_full[r] >= 0).sum() and (dense[r + 1:] < 0).all()
    gm = ctx.detect_u8(img, 0)
    assert_detect_equal(orc, ctx, om, gm, f"checkerboard cut at {kmax}")
    assert_field_equal(orc, om, gm, f"checkerboard cut at {kmax}")
    gm.release()
    ctx.close()


# ---- e. the batch spelling of the candidate test ------------------------------------------------------------------------------
BATCH_CONFIGS = {
    "pos_neg_threshold=0.12": dict(BASE, pos_neg_threshold=0.12),
    "dog_threshold=0.3": dict(BASE, dog_threshold=0.3),
    "servo-swing": servo_kw("swing"),
    "combined": dict(BASE, **COMBINED),
}
BATCH_STEPS = 10


def lane_orders(lanes):
    """different orders of the twelve frames per lane, so that the lanes' counts and servo states differ"""
    return [list(range(BATCH_STEPS)), list(range(11, 11 - BATCH_STEPS, -1)), [(5 * k + 2) % 12 for k in range(BATCH_STEPS)]][:lanes]


def batch_run(B, params, lanes, streams, steps):
    """streams[l][k] = lane l's frame at step k: every lane's (record words, keyline count) per pair, and its detector state"""
    H, W = params.rows, params.cols
    bat = B.Batch(params, lanes)
    devs = [bat.lanes[l].upload_frames(streams[l]) for l in range(lanes)]
    got = [[] for _ in range(lanes)]
    for k in range(steps):
        outs, nks = bat.push_u8_device([d + k * H * W for d in devs], k * 50000)
        for l in range(lanes):
            if outs[l].status >= 0:
                got[l].append((record_words(outs[l]), int(nks[l])))
    for outs, nks in bat.flush():
        for l in range(lanes):
            got[l].append((record_words(outs[l]), int(nks[l])))
    states = [bat.lanes[l].detector_state() for l in range(lanes)]
    bat.close()
    return got, states


def alone_run(B, params, frames, steps):
    ctx = B.Context(params)
    dev = ctx.upload_frames(frames)
    recs = [(record_words(o), int(n)) for o, n in run_stream(ctx, dev, range(steps), params.rows * params.cols)]
    state = ctx.detector_state()
    ctx.close()
    return recs, state


def assert_lane_equals_alone(got, state, alone, alone_state, what):
    assert len(got) == len(alone), (what, len(got), len(alone))
    for k, ((wg, ng), (wa, na)) in enumerate(zip(got, alone)):
        assert ng == na, (what, k, ng, na)
        assert np.array_equal(wg, wa), (what, k, np.flatnonzero(wg != wa)[:8])
    assert np.array_equal(_bits(state[:2]), _bits(alone_state[:2])) and state[2] == alone_state[2], (what, state, alone_state)


@pytest.mark.parametrize("lanes,head", [(3, None), (2, "compact1")], ids=["3-lanes", "2-lanes-compact1"])
@pytest.mark.parametrize("config", list(BATCH_CONFIGS))
def test_batch_lanes_off_the_defaults(orc_mod, B, small_stream, monkeypatch, config, lanes, head):
    """Batches run the candidate test as keyline_flag_body behind k_dog_mag_b, stand-alone contexts as keyline_flag_ii_body: every
    lane's records, keyline counts and detector state equal those of a stand-alone context fed the same frames, and (servo-swing)
    those of the oracle with its sums in the kernels' order."""
    frames, cam = small_stream
    kw = dict(BATCH_CONFIGS[config], global_min_matches_threshold=1)
    orders = lane_orders(lanes)
    streams = [np.ascontiguousarray(frames[o]) for o in orders]
    set_forms(monkeypatch, batch_head=head)
    got, states = batch_run(B, params_for(B, cam, **kw), lanes, streams, BATCH_STEPS)
    set_forms(monkeypatch)
    for l in range(lanes):
        alone, alone_state = alone_run(B, params_for(B, cam, **kw), streams[l], BATCH_STEPS)
        assert len(alone) == BATCH_STEPS - 1
        assert_lane_equals_alone(got[l], states[l], alone, alone_state, f"{config} lane {l}")
    assert [n for _, n in got[0]] != [n for _, n in got[1]]
    if config == "servo-swing":
        for l in range(lanes):
            orc = orc_mod.Oracle(params_for(orc_mod, cam, **kw))
            orc.set_sum_order("device")
            prev = None
            for k in range(BATCH_STEPS):
                m = orc.detect_u8(streams[l][k], k * 50000)
                if prev is not None:
                    wo = record_words(orc.track_pair(prev, m))
                    assert got[l][k - 1][1] == m.size(), (l, k, got[l][k - 1][1], m.size())
                    assert np.array_equal(got[l][k - 1][0], wo), ("oracle", l, k, np.flatnonzero(got[l][k - 1][0] != wo)[:8])
                prev = m
            thr, auto, cnt = states[l]
            assert np.array_equal(_bits([thr, auto]), _bits([orc.threshold, orc.auto_threshold])) and cnt == prev.size()


@pytest.mark.parametrize("gate", ["magnitude", "gradient"])
def test_batch_gate_at_equality(orc_mod, B, small_stream, gate):
    """The eight bounds of test_gate_at_equality through the batch spelling: a 2-lane batch with the parameter on the value and one
    ulp above it, frame 0 (where the values were read) as the second frame of both lanes; the count that comes with the record
    and the detector's count must be the oracle's."""
    frames, cam = small_stream
    name, cases, _, _ = equality_cases(orc_mod, small_stream, gate)
    streams = [np.ascontiguousarray(frames[[1, 0]]), np.ascontiguousarray(frames[[2, 0]])]
    for v, t, on, above in cases:
        for p, want in ((t, on), (np.nextafter(t, F32(np.inf)), above)):
            got, states = batch_run(B, params_for(B, cam, **dict(BASE, **{name: float(p)})), 2, streams, 2)
            for l in range(2):
                assert [n for _, n in got[l]] == [want] and states[l][2] == want, (gate, v, p, l, got[l][0][1], states[l], want)


def test_batch_lanes_on_crafted_images(orc_mod, B):
    """The crafted images are no streams (a frame repeated gives a degenerate pair): lane against stand-alone context on the
    keyline counts and the detector state only, the checkerboard in one lane, the star in the next, the bar in the third; the
    counts are the oracle's."""
    W, H = 131, 67
    steps = 3
    imgs = [IMAGES[n](W, H) for n in ("checkerboard", "star", "bar")]
    want = [orc_mod.Oracle(orc_mod.default_params(H, W, **KW_IMG)).detect_u8(img, 0).size() for img in imgs]
    streams = [np.ascontiguousarray(np.stack([img] * steps)) for img in imgs]
    got, states = batch_run(B, B.default_params(H, W, **KW_IMG), 3, streams, steps)
    for l in range(3):
        alone, alone_state = alone_run(B, B.default_params(H, W, **KW_IMG), streams[l], steps)
        assert [n for _, n in got[l]] == [n for _, n in alone] == [want[l]] * (steps - 1), (l, got[l], want[l])
        assert np.array_equal(_bits(states[l][:2]), _bits(alone_state[:2])) and states[l][2] == alone_state[2] == want[l], (l, states[l], alone_state)
