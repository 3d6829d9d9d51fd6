"""The lens front end on the CPU: the oracle's cv::undistort restatement (orc_front_end_u8), the host map function the device
gathers through (hm::undistort_fixed_map) and rebvio::Camera::undistort against the longdouble statement of tests/lens_cases.py,
on cameras with fx != fy, principal points off the centre, near a corner and outside the image, and on pixels planted at the
gather's edges and beyond what a short and an int hold.

No comparison here has a tolerance or leaves a pixel out. What makes that legitimate is a condition on the inputs: every
camera keeps every pixel's 32 u and 32 v at least MIN_TIE = 1e-6 away from a half-integer (in longdouble), a thousand times the
rounding error a double evaluation of the map has at these sizes, so rint of any correct evaluation is the same word.
test_every_camera_keeps_away_from_ties asserts it for every case the CPU and GPU tests use."""
import os
import subprocess

import numpy as np
import pytest

import lens_cases as lc
from support import ROOT, host_lib, host_math_tool, noise_frames  # noqa: F401


def all_map_cases():
    """every case whose map is compared word for word, here or in tests/test_lens_front_end_gpu.py"""
    cases = {name: case for name, case in lc.CAMERAS.items()}
    for name in lc.SMALL:
        for cols, rows in lc.MAP_SIZES:
            cases[f"{name}@{cols}x{rows}"] = lc.at_size(lc.CAMERAS[name], cols, rows)
    for cols in lc.STRIPE_WIDTHS:
        cases[f"stripes-{cols}"] = lc.stripe_case(cols)
        cases[f"stripes-{cols}x7"] = lc.stripe_case(cols, 7)       # below what a context takes: the host map program alone
    return cases


def oracle_for(orc_mod, case):
    cols, rows, fx, fy, cx, cy, _ = case
    return orc_mod.Oracle(orc_mod.default_params(rows, cols, fm=0.5 * (fx + fy), cx=cx, cy=cy))


def oracle_front_end(orc_mod, case, frame):
    return oracle_for(orc_mod, case).front_end_u8(frame, *lc.K4(case), lc.D5(case))


def test_every_camera_keeps_away_from_ties():
    """The condition under which the maps are compared word for word, and that the table holds what it is meant to hold."""
    for name, case in all_map_cases().items():
        assert lc.min_tie(case) > lc.MIN_TIE, (name, lc.min_tie(case))
    C = lc.CAMERAS
    assert all(C[n][2] != C[n][3] for n in ("euroc-quarter", "pincushion-150-140", "euroc-full"))
    assert C["pincushion-150-140"][2:4] == (150.0, 140.0)
    cols, rows, _, _, cx, cy, D = C["corner-principal-point"]
    assert (cx, cy) == (20.25, rows - 19.25) and D[2] != 0 and D[3] != 0
    cols, rows, _, _, cx, cy, _ = C["principal-point-outside"]
    assert not (0 <= cx < cols and 0 <= cy < rows)
    iu, iv = lc.map_words(C["nearly-identity"])
    j, i = np.meshgrid(np.arange(255), np.arange(255))
    assert np.array_equal(iu, 32 * j) and np.array_equal(iv, 32 * i)          # the gather runs, every pixel reads itself
    assert C["tangential-only"][6][:2] == (0.0, 0.0) and C["tangential-only"][6][4] == 0.0
    for name in ("pincushion-150-140", "corner-principal-point", "principal-point-outside"):   # these reach outside the frame
        assert not lc.inside(*lc.map_words(C[name]), C[name][0], C[name][1]).all(), name


@pytest.mark.parametrize("name", lc.SMALL)
def test_oracle_map_equals_the_direct_statement(orc_mod, name):
    """The oracle's map read back through the ramp frames, at the camera's own size and at the four sizes the GPU test runs:
    word for word rint(direct_map) where all four taps are inside, and the zero-border bilinear formula of those words on
    every pixel of both frames."""
    differing = 0
    for case in [lc.CAMERAS[name]] + [lc.at_size(lc.CAMERAS[name], c, r) for c, r in lc.MAP_SIZES]:
        assert lc.min_tie(case) > lc.MIN_TIE, (name, case[:2])
        cols, rows = case[:2]
        iu, iv = lc.map_words(case)
        inside = lc.inside(iu, iv, cols, rows)
        assert inside.sum() > cols * rows // 4, (name, case[:2])
        orc = oracle_for(orc_mod, case)
        for ramp, words, axis in zip(lc.ramp_frames(cols, rows), (iu, iv), "uv"):
            out = orc.front_end_u8(ramp, *lc.K4(case), lc.D5(case))
            got, exact = lc.decode_ramp(out)
            differing += int((got != words)[inside].sum())
            assert exact[inside].all() and np.array_equal(got[inside], words[inside]), (name, case[:2], axis)
            assert np.array_equal(out.view(np.uint32), lc.remap(iu, iv, ramp).view(np.uint32)), (name, case[:2], axis)
    print(name, "differing map words:", differing)


@pytest.mark.parametrize("name", ["euroc-full"] + [f"stripes-{w}" for w in lc.STRIPE_WIDTHS])
def test_oracle_on_wide_frames_equals_the_direct_statement(orc_mod, name):
    """Wider than a ramp can decode: the image of the (7 col + 13 row) & 255 frame, every pixel, against the zero-border formula
    of rint(direct_map). Stripes of 5, 3, 2 and 1 rows, the last one ragged."""
    case = all_map_cases()[name]
    assert lc.min_tie(case) > lc.MIN_TIE
    frame = lc.weave_frame(*case[:2])
    out = oracle_front_end(orc_mod, case, frame)
    assert np.array_equal(out.view(np.uint32), lc.remap(*lc.map_words(case), frame).view(np.uint32)), name


@pytest.mark.parametrize("name", list(lc.PLANTS))
def test_planted_pixels_saturate_in_the_oracle(orc_mod, name):
    """A pixel sent past what a short (and an int) holds reads the border, as OpenCV's twice saturated map makes it; a pixel
    planted on an edge of the gather reads exactly the taps that are inside, with the weights of its fraction."""
    case, (row, col), (iu, iv) = lc.planted(name)
    cols, rows = case[:2]
    frames = [np.full((rows, cols), 200, np.uint8), np.maximum(noise_frames(cols, rows, 1, 5)[0], 1)]   # no zero pixel
    for frame in frames:
        out = oracle_front_end(orc_mod, case, frame)
        want = lc.planted_value(name, frame)
        reads = lc.PLANTS[name][2]
        assert (want == 0.0) == (reads == "border"), (name, want)
        assert out[row, col] == want, (name, out[row, col], want)
    px = lambda r, c: int(frames[1][r, c])
    if name == "sx=-1":          # by hand: iu = -16, so only column 0 of row 32, weight 16 / 32
        assert iu == -16 and iv == 32 * 32 and out[row, col] == np.float32(3 * 0.5 * px(32, 0))
    if name == "fraction-31/32":
        assert iu == 10 * 32 + 31 and out[row, col] == np.float32(3 * (px(32, 10) + px(32, 11) * 31) / 32)
    if name == "sy=rows-1":
        assert iv == 63 * 32 + 8 and iu == 48 * 32 and out[row, col] == np.float32(3 * px(63, 48) * 24 / 32)


def non_finite_cases():
    base = lc.CAMERAS["euroc-quarter"]
    cases = {}
    for k, bad in enumerate((np.nan, np.inf, -np.inf, np.nan, -np.inf)):
        D = list(base[6])
        D[k] = bad
        cases[f"D[{k}]={bad}"] = base[:6] + (tuple(D),)
    cases["cx=nan"] = base[:4] + (np.nan,) + base[5:]
    cases["cy=inf"] = base[:5] + (np.inf,) + base[6:]
    return cases


def test_the_host_map_as_a_stand_alone_program_under_sanitizers(tmp_path):
    """tests/cpp/lens_map_host_check.cpp over hostmath.hpp alone, built with AddressSanitizer, UndefinedBehaviorSanitizer and its
    float-cast-overflow check: hm::undistort_fixed_map of every camera (every size, the striped widths at 35 and at 7 rows) equals
    rint(direct_map) word for word; the planted pixels hold their planted words, the ones beyond int's range INT_MAX and
    INT_MIN; NaN and infinite intrinsics convert without undefined behaviour, a NaN to INT_MIN. A program of its own on the CPU;
    nothing of it is loaded into this process."""
    exe = str(tmp_path / "lens_map_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rebvio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "lens_map_host_check.cpp"), "-o", exe], check=True)
    cases = all_map_cases()
    exact = set(cases)
    cases.update({f"planted {n}": lc.planted(n)[0] for n in lc.PLANTS})
    cases.update(non_finite_cases())
    fin, fout = str(tmp_path / "cases.bin"), str(tmp_path / "maps.bin")
    with open(fin, "wb") as f:
        for case in cases.values():
            f.write(np.array(case[:2], np.int32).tobytes())
            f.write(np.array(list(case[2:6]) + list(case[6]), np.float32).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    maps = np.fromfile(fout, np.int32)
    assert maps.size == sum(2 * c[0] * c[1] for c in cases.values())
    at = 0
    for name, case in cases.items():
        cols, rows = case[:2]
        got = maps[at:at + 2 * cols * rows].reshape(rows, cols, 2).astype(np.int64)
        at += 2 * cols * rows
        iu, iv = lc.map_words(case)
        if name in exact:
            assert np.array_equal(got[..., 0], iu) and np.array_equal(got[..., 1], iv), name
        elif name.startswith("planted"):
            _, (row, col), words = lc.planted(name[len("planted "):])
            assert tuple(got[row, col]) == words, (name, got[row, col], words)
        else:   # not finite: NaN -> INT_MIN, +-inf -> the end of int's range on its side, everything else as the statement has it
            wu, wv, du, dv = lc.direct_map(case)
            sure = (du > lc.MIN_TIE) & (dv > lc.MIN_TIE)
            assert np.array_equal(got[..., 0][sure], iu[sure]) and np.array_equal(got[..., 1][sure], iv[sure]), name
            nan_u, nan_v = np.isnan(wu), np.isnan(wv)
            assert (nan_u | nan_v | np.isinf(wu) | np.isinf(wv)).any(), name
            assert (got[..., 0][nan_u] == lc.INT_MIN).all() and (got[..., 1][nan_v] == lc.INT_MIN).all(), name
    assert {lc.INT_MAX, lc.INT_MIN} <= {lc.planted(n)[2][0] for n in lc.PLANTS}


def test_camera_undistort_reads_the_border_too(host_math_tool):  # noqa: F811
    """rebvio::Camera::undistort (rebvio_amd/host/types.cpp) goes through the same map function: a planted pixel beyond a short,
    one beyond an int and one on the left edge read what the oracle reads."""
    for name in ("wrap-65536+10", "beyond-2^31", "beyond--2^31", "sx=-1", "sx=cols-1"):
        case, (row, col), _ = lc.planted(name)
        cols, rows, fx, fy, cx, cy, D = case
        assert fx == fy
        frame = np.maximum(noise_frames(cols, rows, 1, 5)[0], 1)
        img = frame.astype(np.float32) * np.float32(3.0)
        out = host_math_tool("undistort", np.concatenate([np.array([rows, cols, fx, cx, cy, D[0], D[1], D[2], D[3], D[4]], np.float32),
                                                          img.reshape(-1)])).reshape(rows, cols)
        assert out[row, col] == lc.planted_value(name, frame), (name, out[row, col])
