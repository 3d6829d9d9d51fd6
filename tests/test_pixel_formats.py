"""Camera pixel formats on the CPU: the host form of the grey conversion (rebvio_amd/csrc/pixel_format.hpp, the same source the
device front end compiles) against a numpy statement of the format table, and the PNG reader that returns a file's stored
pixels (rebvio::io::readPngPixels) instead of its luma."""
import os
import subprocess

import numpy as np
import pytest

from support import BGR8, BGRA8, BPP, BUILD, GRAY8, INC, RGB8, RGBA8, ROOT, UYVY, YUYV


def luma(r, g, b):
    """cv::cvtColor RGB2GRAY in fixed point (stream_io.cpp's PNG luma, pinned by test_host_api.py)"""
    return ((r.astype(np.int64) * 4899 + g.astype(np.int64) * 9617 + b.astype(np.int64) * 1868 + 8192) >> 14).astype(np.uint8)


def grey_of(frame, fmt):
    """the format table: frame [H, W, bytes per pixel] (or [H, W] for GRAY8) -> grey [H, W]"""
    if fmt == GRAY8:
        return frame if frame.ndim == 2 else frame[..., 0]
    if fmt in (RGB8, RGBA8):
        return luma(frame[..., 0], frame[..., 1], frame[..., 2])
    if fmt in (BGR8, BGRA8):
        return luma(frame[..., 2], frame[..., 1], frame[..., 0])
    return frame[..., 0] if fmt == YUYV else frame[..., 1]  # YUYV: Y0 U Y1 V; UYVY: U Y0 V Y1


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("px") / "pixel_format_dump")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "pixel_format_dump.cpp"), "-o", exe], check=True)
    return exe


def host_convert(exe, tmp_path, frame, fmt):
    rows, cols = frame.shape[:2]
    src, dst = tmp_path / f"in{fmt}.bin", tmp_path / f"out{fmt}.bin"
    np.ascontiguousarray(frame).tofile(src)
    subprocess.run([exe, str(fmt), str(rows), str(cols), str(src), str(dst)], check=True)
    return np.fromfile(dst, np.uint8).reshape(rows, cols)


def test_host_conversion_of_every_rgb_triple(dump_exe, tmp_path):
    """All 2^24 colours, in both byte orders, with and without alpha (alpha random: it must not matter)."""
    v = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    want = luma(rgb[..., 0], rgb[..., 1], rgb[..., 2])
    alpha = np.random.default_rng(1).integers(0, 256, rgb.shape[:2] + (1,), dtype=np.uint8)
    cases = {RGB8: rgb, BGR8: rgb[..., ::-1], RGBA8: np.concatenate([rgb, alpha], -1),
             BGRA8: np.concatenate([rgb[..., ::-1], alpha], -1)}
    for fmt, frame in cases.items():
        assert np.array_equal(grey_of(frame, fmt), want)                      # (the numpy table agrees with itself)
        got = host_convert(dump_exe, tmp_path, frame, fmt)
        assert np.array_equal(got, want), (fmt, np.argwhere(got != want)[:4])
    # the constants: white stays white, the weights sum to 2^14
    assert luma(np.array([255]), np.array([255]), np.array([255]))[0] == 255 and 4899 + 9617 + 1868 == 1 << 14


@pytest.mark.parametrize("cols", [2, 6, 640])
def test_host_conversion_of_packed_yuv_and_grey(dump_exe, tmp_path, cols):
    rng = np.random.default_rng(cols)
    rows = 37
    for fmt in (GRAY8, YUYV, UYVY):
        frame = rng.integers(0, 256, (rows, cols, BPP[fmt]), dtype=np.uint8)
        got = host_convert(dump_exe, tmp_path, frame, fmt)
        assert np.array_equal(got, grey_of(frame, fmt)), fmt
    # YUYV / UYVY: the Y bytes in stream order are the grey row
    frame = rng.integers(0, 256, (rows, cols * 2), dtype=np.uint8)
    assert np.array_equal(host_convert(dump_exe, tmp_path, frame.reshape(rows, cols, 2), YUYV), frame[:, 0::2])
    assert np.array_equal(host_convert(dump_exe, tmp_path, frame.reshape(rows, cols, 2), UYVY), frame[:, 1::2])


@pytest.fixture(scope="module")
def png_exe(tmp_path_factory):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "rebvio_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "rebvio_amd", "host")], check=True)
    exe = str(tmp_path_factory.mktemp("png") / "png_pixels_dump")
    subprocess.run(["g++", "-std=c++17", "-O1"] + INC + [os.path.join(ROOT, "tests", "cpp", "png_pixels_dump.cpp"), "-o", exe,
                    "-L", BUILD, "-lrebvio", "-lrebvio_hip", f"-Wl,-rpath,{BUILD}", "-pthread"], check=True)
    return exe


def read_pixels(exe, path, opencv=False):
    out = str(path) + ".dump"
    subprocess.run([exe, str(path), out] + (["opencv"] if opencv else []), check=True)
    raw = np.fromfile(out, np.uint8)
    fmt, rows, cols, cvtype = raw[:16].view(np.int32)
    return int(fmt), int(cvtype), raw[16:].reshape(rows, cols, -1)


@pytest.mark.parametrize("shape", [(40, 64), (23, 31)])
def test_png_reader_returns_the_stored_pixels(png_exe, tmp_path, shape):
    """RGB8, RGBA8 and grey8 PNGs, every row filter (None, Sub, Up, Average, Paeth) in turn: the reader gives back the written
    bytes with their format code and cv::Mat type; with OpenCV's order R and B are swapped (what cv::imread returns)."""
    from pngutil import write_png
    rng = np.random.default_rng(sum(shape))
    H, W = shape
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    rgb[: H // 2] = (np.arange(W, dtype=np.uint8)[None, :, None] * np.array([3, 5, 7], np.uint8))  # smooth rows: real predictions
    rgba = np.concatenate([rgb, rng.integers(0, 256, (H, W, 1), dtype=np.uint8)], -1)
    grey = rng.integers(0, 256, (H, W), dtype=np.uint8)
    cases = [("rgb", rgb, RGB8, BGR8, 16), ("rgba", rgba, RGBA8, BGRA8, 24), ("grey", grey, GRAY8, GRAY8, 0)]
    for name, img, fmt, fmt_cv, cvtype in cases:
        p = tmp_path / f"{name}.png"
        write_png(str(p), img, filters=(0, 1, 2, 3, 4))
        f, t, px = read_pixels(png_exe, p)
        assert (f, t) == (fmt, cvtype), name
        assert np.array_equal(px.reshape(img.shape), img), name
        f, t, px = read_pixels(png_exe, p, opencv=True)
        want = img.copy()
        if img.ndim == 3:
            want[..., [0, 2]] = img[..., [2, 0]]
        assert (f, t) == (fmt_cv, cvtype) and np.array_equal(px.reshape(img.shape), want), name
        if img.ndim == 3:  # OpenCV order through the format table = the luma readPngGray returns
            assert np.array_equal(grey_of(px.reshape(img.shape), fmt_cv), luma(img[..., 0], img[..., 1], img[..., 2]))
