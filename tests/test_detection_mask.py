"""Detection masks on the CPU: the header declares the new entries with the documented signatures, the Python binding lists them,
a grey PNG mask round-trips through the stored-pixel reader rebvio_replay --mask uses, and rebvio_replay --mask without a file
name stops at its usage line before it opens a device."""
import os
import re
import subprocess

import numpy as np
import pytest

from support import BUILD, INC, ROOT


DECLS = {
    "rebvio_hip_set_detection_mask": "int rebvio_hip_set_detection_mask(rebvio_hip_ctx* ctx, const uint8_t* mask_host, size_t pitch_bytes);",
    "rebvio_hip_detect_px_masked_device": "int rebvio_hip_detect_px_masked_device(rebvio_hip_ctx* ctx, const void* frame_dev, int fmt, "
                                          "const uint8_t* mask_dev, uint64_t ts_us, rebvio_hip_map** out);",
    "rebvio_hip_push_frame_px_masked_device": "int rebvio_hip_push_frame_px_masked_device(rebvio_hip_ctx* ctx, const void* frame_dev, "
                                              "int fmt, const uint8_t* mask_dev, uint64_t ts_us, rebvio_hip_pair_out* out, int* keylines);",
    "rebvio_hip_batch_push_px_masked_device": "int rebvio_hip_batch_push_px_masked_device(rebvio_hip_batch* b, const void* const* "
                                              "frames_dev, int fmt, const uint8_t* const* masks_dev, uint64_t ts_us, rebvio_hip_pair_out* "
                                              "out, int* keylines);",
}


def _header_decls():
    text = open(os.path.join(ROOT, "include", "rebvio_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return {m.group(1): re.sub(r"\s+", " ", m.group(0)).replace("( ", "(")
            for m in re.finditer(r"\bint\s+(rebvio_hip_\w+)\s*\([^;]*\);", text)}


def test_header_declares_the_mask_entries():
    decls = _header_decls()
    for name, want in DECLS.items():
        assert decls.get(name) == want, (name, decls.get(name))
    text = open(os.path.join(ROOT, "include", "rebvio_hip.h")).read()
    assert "#define REBVIO_HIP_ABI_VERSION 3" in text
    for word in ("UNDISTORTED", "non-zero", "NULL clears", "handed out"):
        assert word in text, word


def test_binding_lists_the_mask_entries():
    from rebvio_amd import backend
    for name in DECLS:
        assert name in backend.SIGNATURES, name
    assert len(backend.SIGNATURES["rebvio_hip_batch_push_px_masked_device"][1]) == 7


@pytest.fixture(scope="module")
def host_build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "rebvio_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "rebvio_amd", "host")], check=True)
    return BUILD


@pytest.mark.parametrize("shape", [(48, 64), (23, 31)])
def test_grey_png_mask_round_trips(host_build, tmp_path, shape):
    """A 0 / 255 mask (and one of arbitrary bytes) written as a grey PNG comes back from readPngPixels as the same CV_8UC1 bytes."""
    from pngutil import write_png
    exe = str(tmp_path / "png_pixels_dump")
    subprocess.run(["g++", "-std=c++17", "-O1"] + INC + [os.path.join(ROOT, "tests", "cpp", "png_pixels_dump.cpp"), "-o", exe,
                    "-L", host_build, "-lrebvio", "-lrebvio_hip", f"-Wl,-rpath,{host_build}", "-pthread"], check=True)
    H, W = shape
    rng = np.random.default_rng(H)
    masks = [np.where(rng.random((H, W)) < 0.5, 255, 0).astype(np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)]
    masks[0][: H // 3] = 0
    for k, m in enumerate(masks):
        p = tmp_path / f"mask{k}.png"
        write_png(str(p), m, filters=(0, 1, 2, 3, 4))
        out = str(p) + ".dump"
        subprocess.run([exe, str(p), out], check=True)
        raw = np.fromfile(out, np.uint8)
        fmt, rows, cols, cvtype = raw[:16].view(np.int32)
        assert (fmt, rows, cols, cvtype) == (0, H, W, 0)
        assert np.array_equal(raw[16:].reshape(H, W), m)


def test_replay_mask_without_a_file_name_prints_usage(host_build, tmp_path):
    exe = os.path.join(host_build, "rebvio_replay")
    for args in (["--mask"], ["--raw", str(tmp_path / "x.u8"), "--size", "64", "48", "--mask", "--out", str(tmp_path / "o.txt")]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
        assert r.stderr.startswith("usage:") and "--mask mask.png" in r.stderr, r.stderr
    assert not (tmp_path / "o.txt").exists()
