#!/usr/bin/env python3
"""Per-kernel resource table from the gfx950 assembly that `hipcc --save-temps` leaves beside a source
(<stem>-hip-amdgcn-amd-amdhsa-gfx950.s): VGPRs, SGPRs, LDS and scratch bytes, static instruction count and the number of
scratch_ (vector spill / private memory) instructions. Needs no GPU.

    python tools/codeobj_table.py [--grep TEXT] FILE.s [FILE.s ...]

Kernels are named by their demangled symbol; --grep keeps those whose name contains TEXT.
"""
from __future__ import annotations

import argparse
import re
import shutil
import subprocess

FIELDS = (("vgpr", r"; NumVgprs: (\d+)"), ("sgpr", r"; TotalNumSgprs: (\d+)"), ("lds", r"; LDSByteSize: (\d+)"),
          ("scratch", r"; ScratchSize: (\d+)"))
INSTR = re.compile(r"^\t([a-z][a-z0-9_]+)(\s|$)")


def demangle(names):
    exe = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    out = subprocess.run([exe], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return [re.sub(r"\(anonymous namespace\)::", "", o).split("(")[0].replace("void ", "") for o in out[:len(names)]]


def kernels(path):
    """[(symbol, {field: int, "instr": int, "scratch_instr": int})] in file order"""
    text = open(path).read()
    res = []
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)$", text, re.M):
        sym = m.group(1)
        start = text.index(f"\n{sym}:")
        body = text[start:text.index("\n.Lfunc_end", start)]
        ops = [i.group(1) for i in map(INSTR.match, body.split("\n")) if i]
        tail = text[text.index(body) + len(body):]
        row = {k: int(re.search(rx, tail).group(1)) for k, rx in FIELDS}
        row["instr"] = len(ops)
        row["scratch_instr"] = sum(o.startswith("scratch_") for o in ops)
        res.append((sym, row))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="+")
    ap.add_argument("--grep", default="")
    a = ap.parse_args()
    for f in a.files:
        ks = kernels(f)
        names = demangle([s for s, _ in ks])
        print(f"# {f}")
        print(f"{'kernel':<64}{'VGPR':>6}{'SGPR':>6}{'LDS':>8}{'scratch':>9}{'instr':>8}{'scratch_*':>10}")
        for name, (_, r) in zip(names, ks):
            if a.grep in name:
                print(f"{name:<64}{r['vgpr']:>6}{r['sgpr']:>6}{r['lds']:>8}{r['scratch']:>9}{r['instr']:>8}{r['scratch_instr']:>10}")


if __name__ == "__main__":
    main()
