#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 assembly of kernels/wavefront.hip in two source trees (no GPU needed):
    python3 tools/kernel_asm_diff.py <tree A> <tree B> [filter regex [kernel file, kernels/wavefront.hip by default]]
Each tree's file is compiled with its own Makefile's HIPFLAGS plus -S --cuda-device-only, from its csrc directory, so the file name - which
the HIP compilation-unit id is derived from - is the same in both.  The assembly is split by function label and stripped of comments;
per function the output says `identical`, or gives the two instruction counts and the number of differing lines.  Text only: nothing
here knows one instruction from another."""
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

CSRC = "metal-pathtracer-arm64_amd/csrc"


def assembly(tree, source="kernels/wavefront.hip"):
    csrc = os.path.join(tree, CSRC)
    show = ["make", "-s", "--no-print-directory", "--eval", "kernel-asm-flags: ; @echo $(HIPCC) $(HIPFLAGS)", "kernel-asm-flags"]
    flags = subprocess.run(show, cwd=csrc, check=True, capture_output=True, text=True).stdout.split()
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "kernel.s")
        subprocess.run(flags + ["-S", "--cuda-device-only", source, "-o", out], cwd=csrc, check=True)
        with open(out) as f:
            return f.read()


def functions(text):
    """{demangled name: [lines]} - comments, blank lines and the numbering of local labels removed"""
    found, name = {}, None
    for raw in text.splitlines():
        begin = re.match(r"\s*\.type\s+(\S+),@function", raw)
        if begin:
            name = begin.group(1)
            found[name] = []
            continue
        if name is None:
            continue
        if re.match(r"\.Lfunc_end\d+:", raw):
            name = None
            continue
        line = re.sub(r"\.LBB\d+_", ".LBB_", raw.split(";")[0]).strip()
        if line:
            found[name].append(line)
    names = list(found)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return {p: found[n] for n, p in zip(names, plain)}


def instructions(lines):
    return sum(1 for l in lines if not l.startswith(".") and not l.endswith(":"))


def differing(a, b):
    if len(a) == len(b):
        return sum(1 for x, y in zip(a, b) if x != y)
    ops = difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes()
    return sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in ops if tag != "equal")


def main():
    pattern = re.compile(sys.argv[3] if len(sys.argv) > 3 else ".")
    with ThreadPoolExecutor(2) as pool:
        a, b = (functions(t) for t in pool.map(lambda tree: assembly(tree, *sys.argv[4:5]), sys.argv[1:3]))
    for name in sorted(set(a) | set(b)):
        if not pattern.search(name):
            continue
        if name not in a or name not in b:
            print("%-110s only in %s" % (name[:110], sys.argv[1] if name in a else sys.argv[2]))
        elif a[name] == b[name]:
            print("%-110s identical" % name[:110])
        else:
            print("%-110s instructions %6d -> %6d, %5d of %6d lines differ" %
                  (name[:110], instructions(a[name]), instructions(b[name]), differing(a[name], b[name]), len(a[name])))


if __name__ == "__main__":
    main()
