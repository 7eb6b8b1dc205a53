"""The loader every ctypes binding of the package shares: one shared library, found through an environment variable or next to
the package, loaded once, every declared entry point given its signature, and the library's own error string behind check().

There is deliberately NO fallback: a missing library, one that lacks a declared symbol, or a failed call is a RuntimeError
(callers in the reference catch ``Exception`` and break their loop, so errors must be exceptions, never aborts).  Nothing here
imports torch or numpy, so a binding built on it can be exercised on a machine without a GPU.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))


class Binding:
    """`env`: the variable that may name another build of the same ABI (read now, once); `default`: the file name next to the
    package; `prefix`: the three letters every entry point starts with; `table`: {symbol: (restype, argtypes)}.
    <prefix>_last_error and <prefix>_version are part of every library and are added unless the table places them itself."""

    def __init__(self, env, default, prefix, table):
        self.path = os.environ.get(env, os.path.join(HERE, default))
        self.prefix = prefix
        self.table = dict(table)
        self.table.setdefault(prefix + "_last_error", (C.c_char_p, []))
        self.table.setdefault(prefix + "_version", (C.c_int, []))
        self.symbols = list(self.table)
        self._lib = None
        self._lock = threading.Lock()

    def lib(self):
        """Load (once) and return the library; raises RuntimeError if it is not built or lacks a declared symbol."""
        if self._lib is None:
            with self._lock:
                if self._lib is None:
                    self._lib = self._load()
        return self._lib

    def _load(self):
        if not os.path.exists(self.path):
            raise RuntimeError(
                "ubresnet_amd: HIP extension %s is missing; build it with "
                "`python -m ubresnet_amd.build` (hipcc, gfx950). There is no CPU fallback." % self.path)
        try:
            l = C.CDLL(self.path)
        except OSError as e:
            raise RuntimeError("ubresnet_amd: cannot load %s: %s" % (self.path, e))
        missing = [s for s in self.table if not hasattr(l, s)]
        if missing:
            raise RuntimeError("ubresnet_amd: %s lacks symbols: %s" % (self.path, missing))
        for name, (restype, argtypes) in self.table.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = restype, argtypes
        return l

    def check(self, rc: int, what: str = ""):
        if rc != 0:
            msg = getattr(self.lib(), self.prefix + "_last_error")().decode("utf-8", "replace")
            raise RuntimeError("ubresnet_amd HIP call failed (%d) %s: %s" % (rc, what, msg))

    def version(self) -> int:
        return getattr(self.lib(), self.prefix + "_version")()
