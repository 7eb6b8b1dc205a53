#!/usr/bin/env python3
"""List the GPU kernels compiled into the built library, from the symbol table of its gfx950 code object.

kernels(lib) extracts the code object as tools/check_store_hazard.py does (llvm-objdump --offloading on a copy), reads its symbol
table (llvm-objdump -t: every kernel has a descriptor symbol `<mangled name>.kd`) and returns the sorted demangled names in the
normal form normalize() gives: `conv_pc_kernel<float, 4, 2, 9>`, `bn_finalize_kernel` -- no return type, no anonymous
namespace, no parameter list.  Nothing but names is read.

usage: python tools/kernel_symbols.py [path/to/lib.so]   -> one name per line"""
import os
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
CXXFILT = shutil.which("c++filt") or "/usr/bin/c++filt"


def _strip_params(s):
    """drop the trailing parameter list `(...)` of a demangled function name (template arguments hold no parentheses here)"""
    if not s.endswith(")"):
        return s
    depth = 0
    for i in range(len(s) - 1, -1, -1):
        depth += s[i] == ")"
        depth -= s[i] == "("
        if depth == 0:
            return s[:i]
    return s


def normalize(names):
    """mangled or demangled kernel names -> normal form (see the module docstring); one c++filt process for the whole list"""
    names = [n.strip() for n in names if n.strip()]
    if not names:
        return []
    out = subprocess.run([CXXFILT], input="\n".join(names) + "\n", check=True, capture_output=True, text=True).stdout.split("\n")
    res = []
    for s in out[:len(names)]:
        s = _strip_params(s.strip())
        if s.startswith("void "):
            s = s[5:]
        res.append(s.replace("(anonymous namespace)::", "").strip())
    return res


def kernels(lib):
    """-> sorted list of the normalized names of every kernel in `lib`'s gfx950 code object"""
    tmp = tempfile.mkdtemp(prefix="ubr_ks_")
    try:
        so = os.path.join(tmp, "lib.so")
        shutil.copy(lib, so)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        mangled = set()
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" not in f:
                continue
            tab = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-t", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
            for line in tab.split("\n"):
                parts = line.split()
                if parts and parts[-1].endswith(".kd"):
                    mangled.add(parts[-1][:-3])
        return sorted(set(normalize(sorted(mangled))))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for k in kernels(sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "ubresnet_amd", "libubresnet_hip.so")):
        print(k)
