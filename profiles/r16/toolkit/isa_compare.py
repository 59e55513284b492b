#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel.

    python profiles/r16/toolkit/isa_compare.py PARENT_CSRC HEAD_CSRC FILE.hip[:HEADFILE.hip ...] ...

Each FILE.hip is compiled from both trees with the Makefile's HIPFLAGS, once
plain (the product library's form) and once with -DLZF_DIAG (the diagnostic
library's), to device assembly and to the kernel-resource-usage remarks.  A
kernel that moved between files is found by giving the head side more files:
`lzf_lane.hip:lzf_lane.hip+lzf_lane_diag.hip`; a file that only the
diagnostic library compiles is given as `diag:lzf_wparse.hip`.  Every kernel's instruction
stream is normalised (directives, comments and .LBB label numbers dropped) and
compared; the output is the markdown table of isa.md.  No GPU is needed.
"""
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function",
         "-munsafe-fp-atomics"]


def compile_one(csrc, name, defs, tmp):
    """{kernel: (normalised lines, resources)} of one file of one tree"""
    inc = ["-I" + csrc, "-I" + os.path.join(csrc, "..", "..", "include")]
    out = os.path.join(tmp, "k.s")
    r = subprocess.run([HIPCC] + FLAGS + inc + defs + ["--cuda-device-only", "-S",
                       "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, name), "-o", out],
                       capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr)
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: .*?(Function Name|VGPRs|SGPRs|ScratchSize \[bytes/lane\]|"
                      r"Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        elif cur is not None and "AGPR" not in line:
            cur[m.group(1).split()[0]] = m.group(2)
    kernels, name_, body = {}, None, []
    for line in open(out):
        m = re.match(r"(\w+):\s*(;.*)?$", line)
        if m and m.group(1) in res:
            name_, body = m.group(1), []
            continue
        if name_ is None:
            continue
        if line.startswith(".Lfunc_end"):
            kernels[name_] = (body, res[name_])
            name_ = None
            continue
        s = line.split(";")[0].rstrip()
        t = s.strip()
        if not t or (t.startswith(".") and not t.endswith(":")):
            continue
        body.append(re.sub(r"\.LBB\d+_\d+", ".LBB", t))
    return kernels


def demangle(n):
    return subprocess.run(["c++filt", "-p", n], capture_output=True, text=True).stdout.strip() or n


def fmt(r):
    return " / ".join(r.get(k, "?") for k in ("VGPRs", "SGPRs", "ScratchSize", "LDS", "Occupancy"))


def main():
    parent, head, specs = sys.argv[1], sys.argv[2], sys.argv[3:]
    print("| file | build | kernel | parent: lines, VGPR / SGPR / scratch / LDS / occupancy | head | verdict |")
    print("|---|---|---|---|---|---|")
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for spec in specs:
            diag_only = spec.startswith("diag:")
            pf, _, hf = spec[5 if diag_only else 0:].partition(":")
            hfiles = (hf or pf).split("+")
            for build, defs in (("product", []), ("diag", ["-DLZF_DIAG"])):
                if diag_only and not defs:
                    continue
                a = compile_one(parent, pf, defs, tmp)
                b = {}
                for f in hfiles:
                    if f != pf and not defs:
                        continue            # files only the diagnostic library compiles
                    b.update(compile_one(head, f, defs, tmp))
                for k in sorted(set(a) | set(b)):
                    pa, pb = a.get(k), b.get(k)
                    if pa and pb:
                        same = pa[0] == pb[0] and pa[1] == pb[1]
                        verdict = "identical" if same else "DIFFERS (%+d lines)" % (len(pb[0]) - len(pa[0]))
                        bad += (not same) and build == "product"
                    else:
                        verdict = "only in " + ("parent" if pa else "head")
                        bad += build == "product"
                    print("| `%s` | %s | `%s` | %s | %s | %s |" % (
                        pf, build, demangle(k),
                        "%d, %s" % (len(pa[0]), fmt(pa[1])) if pa else "-",
                        "%d, %s" % (len(pb[0]), fmt(pb[1])) if pb else "-", verdict))
    print("\nproduct-build kernels that differ: %d" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
