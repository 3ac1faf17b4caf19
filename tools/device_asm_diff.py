#!/usr/bin/env python3
"""Is the device code of two trees the same?  Compiles clair3_rna_amd/csrc/c3r_lib.hip of each tree for gfx950 (device side only, the
product's flags, no GPU needed) and compares the assembly function by function and kernel descriptor by kernel descriptor.  The order
in which the functions are emitted follows the order in which host code first names them, and the compiler numbers a function's local
labels by that order: both are taken out before comparing.
    python tools/device_asm_diff.py <parent tree> [<this tree>]        exit status 0: identical"""
import os
import re
import subprocess
import sys
import tempfile


def device_asm(root):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "dev.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-function", "--cuda-device-only", "-S",
                               os.path.join(root, "clair3_rna_amd", "csrc", "c3r_lib.hip"), "-o", out])
        return open(out).read()


def parts(asm):
    """{name: text} of every function body and every .amdhsa_kernel block"""
    asm = re.sub(r"\.L(BB|JTI|func_begin|func_end|tmp)\d+", r".L\1", asm)       # (.LBB54_2: block 2 of function 54)
    asm = re.sub(r"\bBB\d+_", "BB_", asm)                                       # (the same in the compiler's loop comments)
    got = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end:", asm, re.S | re.M):
        got[m.group(1)] = m.group(2)
    for m in re.finditer(r"^\t\.amdhsa_kernel (\w+)\n(.*?)^\t\.end_amdhsa_kernel", asm, re.S | re.M):
        got["descriptor of " + m.group(1)] = m.group(2)
    return got


if __name__ == "__main__":
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    a, b = parts(device_asm(sys.argv[1])), parts(device_asm(sys.argv[2] if len(sys.argv) > 2 else here))
    differ = sorted(set(a) ^ set(b)) + sorted(k for k in set(a) & set(b) if a[k] != b[k])
    kernels = sum(1 for k in b if k.startswith("descriptor of "))
    print("%d functions (%d kernels) and their descriptors: %s" % (len(b) - kernels, kernels, "identical" if not differ else "DIFFERENT: " + ", ".join(differ)))
    sys.exit(1 if differ else 0)
