#!/usr/bin/env python3
"""Per-kernel fingerprint of the library's device code: proves that a change which only moves code leaves every kernel's machine
code as it was.  Every csrc/*.hip is compiled to gfx950 assembly with exactly the library's command (keymorph_amd.build: FLAGS +
FILE_FLAGS, `-S --cuda-device-only`); per kernel instance (mangled name) the fingerprint is the sha256 of its instruction text up
to .Lfunc_end -- comments and .loc / .file / .cfi / .p2align lines dropped, .LBB<n>_ renumbered to .LBB_ -- plus its
.amdhsa_kernel ... .end_amdhsa_kernel block (registers, LDS, scratch).
usage: tools/kernel_fingerprint.py [FILE.hip ...] [-DNAME=V ...] > table.tsv
(object, kernel, instruction count, hash; run in both trees, then diff.  Names ending in .hip restrict the run to those units of
csrc/; every other argument goes to the compiler after the library's flags, to fingerprint a build arm such as the fall-back.
--strip-name: the kernel's own symbol inside its text is replaced by a placeholder first, to compare a kernel across a rename --
a non-template kernel that became one instance of a template.)"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from keymorph_amd import build  # noqa: E402


def kernels(txt, strip_name=False):
    for n in re.findall(r'^\s*\.amdhsa_kernel (\S+)', txt, re.M):
        m = re.search(r'^%s:.*?\n(.*?)^\.Lfunc_end\d+:' % re.escape(n), txt, re.S | re.M)
        d = re.search(r'^\s*\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel' % re.escape(n), txt, re.S | re.M)
        body = []
        for line in m.group(1).split('\n'):
            line = line.split(';')[0].strip() if '#ASM' not in line else line.strip()
            if line and not line.startswith(('.loc', '.file', '.cfi', '.p2align')):
                body.append(re.sub(r'\.LBB\d+_', '.LBB_', line))
        desc = [line.strip() for line in d.group(1).split('\n') if line.strip()]
        if strip_name:
            body, desc = [line.replace(n, 'KERNEL') for line in body], [line.replace(n, 'KERNEL') for line in desc]
        yield n, len(body), hashlib.sha256('\n'.join(body + desc).encode()).hexdigest()[:16]


if __name__ == "__main__":
    only = [a for a in sys.argv[1:] if a.endswith(".hip")]
    strip = "--strip-name" in sys.argv[1:]
    extra = [a for a in sys.argv[1:] if not a.endswith(".hip") and a != "--strip-name"]
    for src in build.sources():
        name = os.path.basename(src)
        if only and name not in only:
            continue
        with tempfile.TemporaryDirectory() as td:
            out = os.path.join(td, "k.s")
            subprocess.run([build._hipcc(), *build.FLAGS, *build.FILE_FLAGS.get(name, []), *extra, "-S", "--cuda-device-only", src, "-o", out],
                           check=True, stderr=subprocess.DEVNULL)
            for n, k, h in kernels(open(out).read(), strip):
                print(f"{name}\t{n}\t{k}\t{h}")
