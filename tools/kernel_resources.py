#!/usr/bin/env python3
"""Registers / scratch / occupancy (waves per SIMD) of every kernel, as the compiler reports them
(`hipcc -S --cuda-device-only`): the authoritative source for occupancy -- the register column of a rocprofv3 trace is
not the allocation on gfx950.  Compiled with the library's flags (keymorph_amd.build: FLAGS + FILE_FLAGS).  Usage: tools/kernel_resources.py [file.hip ...] > profiles/rNx_kernel_resources.md"""
import glob
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from keymorph_amd import build  # noqa: E402

ROOT = build.CSRC


def main():
    files = sys.argv[1:] or sorted(glob.glob(os.path.join(ROOT, "*.hip")))
    print("| file | kernel | VGPRs | AGPRs | scratch B | waves / SIMD |\n|---|---|---|---|---|---|")
    for f in files:
        with tempfile.TemporaryDirectory() as td:
            out = os.path.join(td, "k.s")
            # the library's own command (per-file flags included: conv_wgrad.hip and norm.hip are built with max-ILP scheduling)
            subprocess.run([build._hipcc(), *build.FLAGS, *build.FILE_FLAGS.get(os.path.basename(f), []),
                            "--cuda-device-only", "-S", "-o", out, f, "-I", ROOT], check=True, stderr=subprocess.DEVNULL)
            txt = open(out).read()
        for m in re.finditer(r"; Kernel info:.*?\n(.*?); Occupancy: (\d+)", txt, re.S):
            pass
        # the per-function comment block: "; NumVgprs: N" ... "; Occupancy: K" follows each ".Lfunc_end" of a kernel
        for blk in re.finditer(r"^([_A-Za-z0-9]+):\s*; @\1\n(.*?)^; Occupancy: (\d+)", txt, re.S | re.M):
            name, body, occ = blk.group(1), blk.group(2), blk.group(3)
            if ".amdhsa_kernel " + name not in txt:
                continue
            g = lambda k: (re.findall(r"^; %s: (\d+)" % k, body, re.M) or ["?"])[-1]
            dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
            dem = re.sub(r"\(anonymous namespace\)::", "", dem).split("(")[0].replace("void ", "")
            print(f"| {os.path.basename(f)} | `{dem}` | {g('NumVgprs')} | {g('NumAgprs')} | {g('ScratchSize')} | {occ} |")


if __name__ == "__main__":
    main()
