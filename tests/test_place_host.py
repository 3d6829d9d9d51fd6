"""The statements of place recognition as a stand-alone program under sanitizers (CPU). The classes above the C-ABI and
`rebvio_replay --places` are tested on the GPU in tests/test_place_host_gpu.py."""
import os
import subprocess

from support import ROOT


def test_the_statements_as_a_stand_alone_program_under_sanitizers(tmp_path):
    """tests/cpp/place_host_check.cpp over rebvio_amd/csrc/place.hpp alone, built with AddressSanitizer and
    UndefinedBehaviorSanitizer: keyline tables, signatures, databases and result records in heap buffers of exactly the bytes that
    may be touched, hostile values in every field the signature reads, image sizes up to the largest a context accepts. A program
    of its own on the CPU; nothing of it is loaded into this process."""
    exe = str(tmp_path / "place_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rebvio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "place_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
