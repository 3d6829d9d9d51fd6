"""rebvio::Rebvio's keyframe request and callback, EdgeMap::markKeyframe / keyframeMatches on the GPU
(tests/cpp/test_keyframes.cpp says what it checks)."""
import os
import subprocess

import numpy as np
import pytest

from support import host_lib  # noqa: F401
from support import ROOT


pytestmark = pytest.mark.gpu


def test_keyframe_request_callback_and_edge_map_entries(host_lib, tmp_path):
    from rebvio_amd import synth
    n, W, H = 20, 160, 120
    frames, cam = synth.render_stream(W, H, n)
    ts, gyro, acc = synth.imu_samples(synth.make_scene(0), n, noise_seed=1)
    fp, ip = tmp_path / "frames.u8", tmp_path / "imu.bin"
    frames.tofile(fp)
    rec = np.zeros(len(ts), dtype=[("ts", "<i8"), ("gyro", "<f4", 3), ("acc", "<f4", 3)])
    rec["ts"], rec["gyro"], rec["acc"] = ts, gyro, acc
    rec.tofile(ip)
    exe = str(tmp_path / "keyframes")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_keyframes.cpp"), "-o", exe, "-L", host_lib, "-lrebvio", "-lrebvio_hip",
                    f"-Wl,-rpath,{host_lib}", "-pthread"], check=True)
    r = subprocess.run([exe, str(fp), str(W), str(H), str(n), repr(cam.fm), repr(cam.cx), repr(cam.cy), "600", "800", str(ip), "50", "5"],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-3000:], r.stderr[-2000:])
