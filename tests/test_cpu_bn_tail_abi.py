"""The descriptor calls of the BatchNorm-backward / block-tail family (ubr_bn_bwd, ubr_block_tail_bwd, ubr_block_tail_fwd), without
a GPU: the ctypes mirrors of their five structs are laid out as a C99 compiler lays out the header's, and every rule of the host-side
validation rejects the smallest otherwise-valid descriptor that breaks just that rule (UBR_EINVAL, an error text that names the entry
point and the pass).  Validation runs before any HIP call and dereferences none of the operand pointers, so the operands are one
16-byte-aligned host address.  One rule has no case: the 2 GiB bound on the mask of ubr_block_tail_bwd (npix * C / channels-per-unit
bytes) cannot be the only thing wrong, because c2 is always required and its own 2 GiB bound (16 bytes per unit) is sixteen
times tighter."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from ubresnet_amd import _lib as L

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ubresnet_hip.h")
EINVAL = -1
STRUCTS = (("ubr_pix", L.Pix), ("ubr_bn_site", L.BnSite), ("ubr_bn_bwd_desc", L.BnBwdDesc),
           ("ubr_block_tail_bwd_desc", L.BlockTailBwdDesc), ("ubr_block_tail_fwd_desc", L.BlockTailFwdDesc))
C_NAME = {"pass_": "pass"}          # `pass` is a Python keyword; every other field has the header's name


def test_descriptor_layouts_match_header(tmp_path):
    assert (L.PASS_REDUCE, L.PASS_APPLY, L.PASS_APPLY_FIN, L.PASS_FROZEN) == (0, 1, 2, 3)
    assert C.sizeof(L.Pix) == 16 and C.sizeof(L.BnSite) == 72
    assert C.sizeof(L.BnBwdDesc) == 32 + 4 * 16 + 72
    assert C.sizeof(L.BlockTailBwdDesc) == 32 + 7 * 16 + 8 + 2 * 72
    assert C.sizeof(L.BlockTailFwdDesc) == 24 + 3 * 16 + 8 + 6 * 8 + 2 * 8
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.skip("no C compiler")
    body, want = [], []
    for cname, S in STRUCTS:
        body.append('printf("%%zu\\n", sizeof(%s));' % cname)
        want.append(C.sizeof(S))
        for f, _ in S._fields_:
            body.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, C_NAME.get(f, f)))
            want.append(getattr(S, f).offset)
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n%s\nreturn 0; }\n' % (HDR, "\n".join(body)))
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == want


# ------------------------------------------------------------------------------------------------------------------
# validation table
# ------------------------------------------------------------------------------------------------------------------
_BUF = C.create_string_buffer(64)
A = (C.addressof(_BUF) + 15) & ~15                 # stands for every operand: aligned, never dereferenced
NPIX, CH = 8, 16
R, AP, AF, FZ = L.PASS_REDUCE, L.PASS_APPLY, L.PASS_APPLY_FIN, L.PASS_FROZEN
PASS_NAME = {R: "reduce", AP: "apply", AF: "apply_fin", FZ: "frozen"}
ALL = (R, AP, AF, FZ)
NOT_R = (AP, AF, FZ)


def _site(p):
    """the ubr_bn_site of pass p with all that the pass reads, and nothing else"""
    s = L.BnSite(scale=A, shift=A, mean=A, invstd=A)
    if p == AP:
        s.k1 = s.k2 = A
    else:
        s.red = A
    if p == AF:
        s.dgamma = s.dbeta = A
    return s


def _bn(p):
    d = L.BnBwdDesc(dtype=L.F32, pass_=p, relu=1, C=CH, npix=NPIX, count=float(NPIX), ga=(A, CH), ga2=(A, CH), c=(A, CH), bn=_site(p))
    if p != R:
        d.gc = (A, CH)
    return d


def _tail(p, mask=True):
    """bypass block; gate = the mask, or `out` (reduce / apply only)"""
    d = L.BlockTailBwdDesc(dtype=L.F32, pass_=p, C=CH, npix=NPIX, count=float(NPIX), go=(A, CH), go2=(A, CH), c2=(A, CH), cb=(A, CH),
                           bn2=_site(p), bnb=_site(p))
    if mask:
        d.relu_mask = A
    else:
        d.out = (A, CH)
    if p != R:
        d.g_c2, d.g_sc = (A, CH), (A, CH)
    return d


_FINS = []          # keeps the ubr_bn_fwd_fin structs alive that descriptors point to


def _fin():
    f = L.BnFwdFin(stats=A, gamma=A, beta=A, running_mean=A, running_var=A, num_batches_tracked=A, momentum=0.1, eps=1e-5,
                   scale=A, shift=A, mean=A, invstd=A)
    _FINS.append(f)
    return f


def _fwd(form):
    d = L.BlockTailFwdDesc(dtype=L.F32, C=CH, npix=NPIX, c2=(A, CH), sc=(A, CH), out=(A, CH), relu_mask=A)
    if form == "fin":
        d.count, d.fin2, d.fin_b = float(NPIX), C.pointer(_fin()), C.pointer(_fin())
    else:
        d.mean2 = d.scale2 = d.shift2 = d.mean_b = d.scale_b = d.shift_b = A
    return d


def _show(v):
    """a value as it appears in a case id (no addresses)"""
    if isinstance(v, tuple):
        return "(%s)" % ",".join(_show(x) for x in v)
    return str({A: "A", A + 4: "A+4"}.get(v, v)) if isinstance(v, (int, float, type(None))) else "ptr"


def _set(path, value):
    """mutation: d.<path> = value (through pointers where the path crosses fin2 / fin_b)"""
    def m(d):
        *head, last = path.split(".")
        for h in head:
            d = getattr(d, h)
            if h in ("fin2", "fin_b"):
                d = d.contents
        setattr(d, last, value)
    m.what = "%s=%s" % (path, _show(value))
    return m


def _wide(C_):
    """C channels, dense: the LDS bounds"""
    def m(d):
        d.C = C_
        for f, t in d._fields_:
            if t is L.Pix and getattr(d, f).p:
                getattr(d, f).ps = C_
    m.what = "C=%d" % C_
    return m


def _seq(*ms):
    """one rule that takes more than one field to break"""
    def m(d):
        for x in ms:
            x(d)
    m.what = "+".join(x.what for x in ms)
    return m


CASES = []


def _add(entry, make, passes, mutation, **kw):
    for p in passes:
        CASES.append(pytest.param(entry, make, p, kw, mutation,
                                  id="%s-%s-%s%s" % (entry[4:], PASS_NAME.get(p, p), mutation.what, "".join("-%s%s" % i for i in kw.items()))))


# ---- ubr_bn_bwd
for _op, _ps in (("ga", ALL), ("ga2", ALL), ("c", ALL), ("gc", NOT_R)):
    _add("ubr_bn_bwd", _bn, _ps, _set(_op + ".p", A + 4))                 # check_nhwc per operand: alignment
    if _op != "ga2":
        _add("ubr_bn_bwd", _bn, _ps, _set(_op + ".p", None))              # ... and presence of the required ones
_add("ubr_bn_bwd", _bn, (R,), _set("dtype", 3))                            # the other check_nhwc rules, once per entry point
_add("ubr_bn_bwd", _bn, (R,), _set("npix", 0))
_add("ubr_bn_bwd", _bn, (R,), _set("C", 0))
_add("ubr_bn_bwd", _bn, (R,), _set("C", 14))                               # not a multiple of the 4 channels of an fp32 unit
_add("ubr_bn_bwd", _bn, (R,), _set("ga.ps", 12))                           # pixel stride < C
_add("ubr_bn_bwd", _bn, (R,), _set("ga.ps", 18))                           # 72 bytes: no multiple of 16
_add("ubr_bn_bwd", _bn, (R,), _set("npix", 1 << 27))                       # 2^27 pixels x 64 bytes >= 2 GiB
for _k in ("scale", "shift", "mean", "invstd"):
    _add("ubr_bn_bwd", _bn, ALL, _set("bn." + _k, None))                   # null constants, every pass
_add("ubr_bn_bwd", _bn, (AP,), _set("bn.k1", None))                        # k1 and k2 both
_add("ubr_bn_bwd", _bn, (AP,), _set("bn.k2", None))
_add("ubr_bn_bwd", _bn, (R, AF), _set("bn.red", None))                     # (FROZEN: red is optional)
_add("ubr_bn_bwd", _bn, (AF,), _set("count", 0.5))
_add("ubr_bn_bwd", _bn, (AF,), _wide(8196))                                # 8 C bytes of LDS > 64 KiB
_add("ubr_bn_bwd", _bn, (FZ,), _wide(4100))                                # 1025 units: atomic flush, 16 C bytes > 64 KiB
_add("ubr_bn_bwd", _bn, (R,), _set("pass_", -1))                           # pass out of range
_add("ubr_bn_bwd", _bn, (R,), _set("pass_", 4))

# ---- ubr_block_tail_bwd
T = "ubr_block_tail_bwd"
for _op, _ps in (("go", ALL), ("go2", ALL), ("c2", ALL), ("cb", ALL), ("g_c2", NOT_R), ("g_sc", NOT_R)):
    _add(T, _tail, _ps, _set(_op + ".p", A + 4))
    if _op in ("go", "c2", "g_c2", "g_sc"):                                # g_sc: required on a bypass block
        _add(T, _tail, _ps, _set(_op + ".p", None))
_add(T, _tail, (R, AP), _set("out.p", A + 4), mask=False)
_add(T, _tail, (R, AP), _set("out.p", None), mask=False)
_add(T, _tail, (R,), _set("dtype", -1))
_add(T, _tail, (R,), _set("npix", -8))
_add(T, _tail, (R,), _set("C", 18))
_add(T, _tail, (R,), _set("c2.ps", 8))
_add(T, _tail, (R,), _set("c2.ps", 17))
_add(T, _tail, (R,), _set("npix", 1 << 27))
for _k in ("scale", "shift", "mean", "invstd"):
    _add(T, _tail, ALL, _set("bn2." + _k, None))
for _k in ("mean", "invstd"):
    _add(T, _tail, ALL, _set("bnb." + _k, None))                           # null bnpass constants with cb
_add(T, _tail, NOT_R, _set("bnb.scale", None))                             # bnpass scale required on apply with cb
for _k in ("bn2.k1", "bn2.k2", "bnb.k1", "bnb.k2"):
    _add(T, _tail, (AP,), _set(_k, None))                                  # k1 and k2 both, of both sites
_add(T, _tail, (R, AF, FZ), _set("bn2.red", None))
_add(T, _tail, (R, AF, FZ), _set("bnb.red", None))
_add(T, _tail, (AF, FZ), _seq(_set("relu_mask", None), _set("out", (A, CH))))     # a mask is required: `out` is no substitute
_add(T, _tail, (AF,), _set("count", 0.0))
_add(T, _tail, (AF,), _wide(4100))                                         # 16 C bytes of LDS > 64 KiB
_add(T, _tail, (FZ,), _wide(2052))                                         # 513 units: atomic flush, 32 C bytes > 64 KiB
_add(T, _tail, (R,), _set("pass_", -1))
_add(T, _tail, (R,), _set("pass_", 4))

# ---- ubr_block_tail_fwd (in the pass column: its two forms, the six vectors or the fused finalize)
F = "ubr_block_tail_fwd"
for _op in ("c2", "sc", "out"):
    _add(F, _fwd, ("plain", "fin"), _set(_op + ".p", A + 4))
    _add(F, _fwd, ("plain", "fin"), _set(_op + ".p", None))
_add(F, _fwd, ("plain",), _set("dtype", 7))
_add(F, _fwd, ("plain",), _set("npix", 0))
_add(F, _fwd, ("plain",), _set("C", 6))
_add(F, _fwd, ("plain",), _set("out.ps", 4))
_add(F, _fwd, ("plain",), _set("out.ps", 21))
_add(F, _fwd, ("plain",), _set("npix", 1 << 27))
for _k in ("mean2", "scale2", "shift2", "mean_b", "scale_b", "shift_b"):
    _add(F, _fwd, ("fin",), _set(_k, A))                                    # both forms at once
    _add(F, _fwd, ("plain",), _set(_k, None))                                # bn2's vectors all, bnpass's all or none
_add(F, _fwd, ("plain",), _set("fin_b", C.pointer(_fin())))                  # plain form with a fused bnpass site
for _site_ in ("fin2", "fin_b"):                                           # the fused forward's ok() predicate, both sites
    for _k in ("stats", "gamma", "beta", "scale", "shift", "mean", "invstd", "running_mean", "running_var"):
        _add(F, _fwd, ("fin",), _set("%s.%s" % (_site_, _k), None))
    _add(F, _fwd, ("fin",), _seq(_set(_site_ + ".momentum", -1.0), _set(_site_ + ".num_batches_tracked", None)))   # cumulative averaging
_add(F, _fwd, ("fin",), _set("count", 0.0))
_add(F, _fwd, ("fin",), _wide(2732))                                        # 24 C bytes of LDS > 64 KiB


@pytest.mark.parametrize("entry, make, p, kw, mutation", CASES)
def test_validation_rejects(entry, make, p, kw, mutation):
    lib = L.lib()
    d = make(p, **kw)
    mutation(d)
    rc = getattr(lib, entry)(C.byref(d), None)
    msg = lib.ubr_last_error().decode()
    assert rc == EINVAL, "%d %s" % (rc, msg)
    assert entry in msg, msg
    if entry != F and "pass_" not in mutation.what:
        assert "%s(%s)" % (entry, PASS_NAME[p]) in msg, msg


@pytest.mark.parametrize("entry", ("ubr_bn_bwd", T, F))
def test_null_descriptor_is_rejected(entry):
    lib = L.lib()
    assert getattr(lib, entry)(None, None) == EINVAL
    assert entry in lib.ubr_last_error().decode()
