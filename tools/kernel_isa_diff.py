#!/usr/bin/env python3
"""Are the kernels of two builds the same, instruction for instruction?  (No GPU needed.)

    tools/kernel_isa_diff.py OTHER_TREE [file.hip ...]      default files: detect.hip track.hip

Compiles rebvio_amd/csrc/<file> of this tree and of OTHER_TREE (a checkout of the commit to compare with, e.g. a
`git worktree add`) to gfx950 assembly with the Makefile's flags and compares every function that exists in OTHER_TREE:
instructions and operands, with the compiler's per-function label numbers (.LBB<function>_<block>) normalised, since adding a
kernel to a file renumbers them. Prints one line per file and the names that differ or are new; exit status 1 on a difference."""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "--cuda-device-only", "-S"]


def assembly(tree, name, out):
    src = os.path.join(tree, "rebvio_amd", "csrc")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + ["-I", os.path.join(tree, "include"), "-I", src,
                    os.path.join(src, name), "-o", out], check=True, stderr=subprocess.DEVNULL)
    text = open(out).read()
    code = set(re.findall(r"^\s*\.type\s+(\w+),@function", text, flags=re.M))  # kernels and device functions, not data objects
    funcs, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if m and cur is None and m.group(1) in code:
            cur = m.group(1)
            funcs[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        text = line.split(";")[0].strip()
        if text and (not text.startswith(".") or text.startswith(".L")):
            funcs[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", text))
    return {k: v for k, v in funcs.items() if v}


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    other, files = sys.argv[1], sys.argv[2:] or ["detect.hip", "track.hip"]
    bad = False
    with tempfile.TemporaryDirectory() as d:
        for name in files:
            a = assembly(other, name, os.path.join(d, "a.s"))
            b = assembly(HERE, name, os.path.join(d, "b.s"))
            differ = sorted(k for k in a if a[k] != b.get(k))
            new = sorted(k for k in b if k not in a)
            print(f"{name}: {len(a)} functions in the other tree ({sum(map(len, a.values()))} instructions), "
                  f"{len(a) - len(differ)} identical here, {len(differ)} differ, {len(new)} new")
            for k in differ:
                print("  differs:", k)
            for k in new:
                print("  new:", k, f"({len(b[k])} instructions)")
            bad = bad or bool(differ)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
