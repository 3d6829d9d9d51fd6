"""The layouts of the on-demand entries' device scratch as a stand-alone program under sanitizers (CPU): rebvio_amd/csrc/scratch_layout.hpp
is the one place api.hip takes a scratch's size and its views from."""
import os
import subprocess

from support import ROOT


def test_the_layouts_as_a_stand_alone_program_under_sanitizers(tmp_path):
    """tests/cpp/scratch_layout_check.cpp over scratch_layout.hpp alone, built with AddressSanitizer and UndefinedBehaviorSanitizer:
    every scratch laid out over a heap buffer of exactly the bytes its layout reports, for keylines_max of 1, 255, 256, 257, 1000 and
    65 536; the first and last element of every view written, no two views overlapping, every offset and total equal to the
    expression the entries used before the layouts were stated once, the documented alignments. A program of its own on the CPU;
    nothing of it is loaded into this process."""
    exe = str(tmp_path / "scratch_layout_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rebvio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "scratch_layout_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
