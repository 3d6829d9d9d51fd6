"""rebvio_amd/csrc/edge_segments.hpp alone - the statements the segment kernels and the host hook compile - as a stand-alone program
under AddressSanitizer and UndefinedBehaviorSanitizer (tests/cpp/edge_segments_host_check.cpp says what it checks). A program of its
own on the CPU; nothing of it is loaded into this process."""
import os
import subprocess

from support import ROOT


def test_the_per_point_statements_as_a_stand_alone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "edge_segments_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rebvio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "edge_segments_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
