"""Float64 reference of libubresnet_det.so (include/ubresnet_det.h): Philox4x32-10 restated in uint64 arithmetic, the uniforms,
the standard normal z in float64, the whole rule of ubx_apply on image, label and weight, the error bound of a noisy image
element, and the table of cases that tests/test_gpu_det_exact.py runs -- which tests/test_cpu_det.py holds against the symbol
table of the built library.  numpy only; a helper module for the tests (imported by name; not a conftest).

The bound.  u = 2^-24.  As in tests/loss_ref.py and tests/tta_ref.py each library call (logf, cospif, sinpif) is taken as within
2 ulp, a relative error of at most 4u, and each rounded fp32 operation as half an ulp, a relative error of at most u.  The words,
the uniforms u1, u2 and the angle 2 u2 are exact.  Hats are computed values.

  l^ = logf(u1):          relative 4u           (u1 == 1 gives 0 exactly)
  m^ = fl(-2 l^):         exact (a power of two)
  rad^ = sqrt_rn(m^):     the square root halves the relative error of its argument, 2u, and rounds once, u:  3u
  t^ = cospif / sinpif:   relative 4u           (the argument is taken exactly; 0 at a zero of the function)
  z^ = fl(rad^ t^):       3u + 4u + u = 8u      (Z_REL)
  s^ = fl(sigma z^):      8u + u = 9u  of |sigma z|
  y^ = fl(x gain):        u |x gain|;  nothing for a gain whose bits are those of 1.0f (no multiply)
  out^ = fl(y^ + s^):     u |out|

  bound = C_ACC u ((Z_REL + 1) |sigma z| + [gain != 1] |x gain| + |out|) + FLOOR

(an fp32 product x gain that is an infinity or a NaN stays what it is: no bound), with x, gain, sigma the fp32 numbers, z and out
from the float64 reference, C_ACC = 1.03 for the second-order terms as in kref, and FLOOR = 2^-146 for roundings at the spacing of the subnormals (two products at half a spacing each; the add is exact there).
Derived from the operations as written, never fitted to what the kernel returns: a ratio above 1 is a finding.
"""
import numpy as np

U32 = 2.0 ** -24
C_ACC = 1.03
LIB = 4.0                  # relative error of a library call, in units of u: 2 ulp
Z_REL = LIB / 2 + 1.0 + LIB + 1.0
FLOOR = 2.0 ** -146
Z_MAX = float(np.sqrt(48.0 * np.log(2.0)))      # u1 >= 2^-24: |z| <= sqrt(-2 ln 2^-24)

LANE_PIXELS, BLOCK, MAX_GRID = 4, 256, 1024     # UBX_LANE_PIXELS, UBX_BLOCK, UBX_MAX_GRID
PHILOX_TAG = 0x55425844                         # UBX_PHILOX_TAG
ONE_BITS = 0x3F800000

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)

# kernel (normal form of tools/kernel_symbols.py) -> ids of the cases of tests/test_gpu_det_exact.py that launch it
KERNEL_CASES = {
    "detector_kernel<false>": ["dead-gain", "dead-some-planes", "switches", "unit-gain-specials", "dead-over-specials", "gain-edge-values",
                               "grid-stride"],
    "detector_kernel<true>": ["noise-lit", "noise-all", "noise-repeat", "noise-other-key", "noise-grid-stride"],
}

# (B, P, H, W) of the small cases: the vector path; W % 4 == 0 with three planes; W % 4 != 0 with a partial mask word; two mask
# words, the second partial; nine mask words
SHAPES = [(2, 1, 3, 8), (2, 3, 5, 12), (1, 1, 5, 7), (2, 3, 2, 37), (1, 2, 3, 260)]
STRIDE_SHAPE = (2, 1, 600, 1024)                # more groups than MAX_GRID * BLOCK lanes


def groups(b, h, w):
    return b * h * ((w + LANE_PIXELS - 1) // LANE_PIXELS)


def row_words(w):
    return 1 + (w + 31) // 32


# ------------------------------------------------------------------------------------------------------------------------
# Philox4x32-10 and the normals
# ------------------------------------------------------------------------------------------------------------------------
def philox(k0, k1, c0, c1, c2, c3):
    """ten rounds over arrays (or scalars) of 32-bit values, every product formed in uint64 -> four uint32 arrays"""
    k0, k1, c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in (k0, k1, c0, c1, c2, c3)])
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                       # both factors are below 2^32: no wrap
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LOW, (p0 >> _S32) ^ c3 ^ k1, p0 & _LOW
        k0, k1 = (k0 + _W0) & _LOW, (k1 + _W1) & _LOW
    return tuple(v.astype(np.uint32) for v in (c0, c1, c2, c3))


def uniforms(a, b):
    """(u1 in (0, 1], u2 in [0, 1)) in float64 from a pair of words"""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return ((a >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * U32, (b >> np.uint64(8)).astype(np.float64) * U32


def _trig_pi(x):
    """(cos(pi x), sin(pi x)) for x in [0, 2), exact at the multiples of 1/2: n quarter turns and t in [-1/4, 1/4]"""
    n = np.rint(2.0 * x)
    t = np.pi * (x - 0.5 * n)
    q = n.astype(np.int64) & 3
    c, s = np.cos(t), np.sin(t)
    return np.choose(q, [c, -s, -c, s]), np.choose(q, [s, c, -s, -c])


def pair_normals(a, b):
    """the two float64 normals of a pair of words: (even column, odd column)"""
    u1, u2 = uniforms(a, b)
    rad = np.sqrt(-2.0 * np.log(u1))
    c, s = _trig_pi(2.0 * u2)
    return rad * c, rad * s


def group_normals(seed, seq, group, r, plane):
    """float64 z of the four columns 4 group .. 4 group + 3 of row r of plane `plane` = b * P + p: [..., 4]"""
    w0, w1, w2, w3 = philox(seed, seq, group, r, plane, PHILOX_TAG)
    z0, z1 = pair_normals(w0, w1)
    z2, z3 = pair_normals(w2, w3)
    return np.stack([z0, z1, z2, z3], axis=-1)


def normals(seed, seq, B, P, H, W):
    """float64 z of every element of a [B, P, H, W] batch"""
    ng = (W + 3) // 4
    plane = np.arange(B * P, dtype=np.uint64).reshape(B * P, 1, 1)
    r = np.arange(H, dtype=np.uint64).reshape(1, H, 1)
    g = np.arange(ng, dtype=np.uint64).reshape(1, 1, ng)
    z = group_normals(seed, seq, g, r, plane)             # [B*P, H, ng, 4]
    return z.reshape(B, P, H, ng * 4)[..., :W]


# ------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------
def make_table(gains, dead, junk=False):
    """gains [B, P] fp32, dead [B, P, W] bool -> uint32 [B, P, 1 + ceil(W/32)]; junk: the bits at and beyond W are SET (the
    kernel must ignore them; DetectorEffects never writes them)"""
    dead = np.asarray(dead, dtype=bool)
    B, P, W = dead.shape
    nw = (W + 31) // 32
    full = np.zeros((B, P, 32 * nw), np.uint8)
    full[..., :W] = dead
    if junk:
        full[..., W:] = 1
    t = np.zeros((B, P, 1 + nw), np.uint32)
    t[..., 0] = np.asarray(gains, dtype=np.float32).reshape(B, P).view(np.uint32)
    t[..., 1:] = np.packbits(full, axis=-1, bitorder="little").view("<u4").reshape(B, P, nw)
    return t


def unpack_table(table, W):
    """-> (gain bits uint32 [B, P], dead bool [B, P, W]), bit by bit as the header states it"""
    table = np.asarray(table, dtype=np.uint32)
    c = np.arange(W)
    dead = ((table[..., 1 + (c >> 5)] >> (c & 31).astype(np.uint32)) & 1).astype(bool)
    return table[..., 0].copy(), dead


# ------------------------------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------------------------------
def reference(image, label, weight, table, sigma=0.0, noise_all=False, seed=0, seq=0, dead_label=None, dead_weight=None):
    """ubx_apply.  image fp32 [B, P, H, W]; label int64 / weight fp32 [B, H, W] or None -> dict:
      exact   fp32 [B, P, H, W]: the element after steps 1 and 2, bit for bit -- the result wherever `noisy` is False
      noisy   bool: step 3 applies
      out     float64: the result (x gain + sigma z in float64 where noisy, `exact` elsewhere)
      bound   float64: the bound of the module docstring where noisy, 0 elsewhere
      label, weight: as the call leaves them (None where None was given);  dead_all bool [B, W]"""
    image = np.ascontiguousarray(image, dtype=np.float32)
    B, P, H, W = image.shape
    gbits, dead = unpack_table(table, W)
    assert gbits.shape == (B, P)
    gain = gbits.view(np.float32)
    sigma = np.float32(sigma)
    unit = (gbits == ONE_BITS)[:, :, None, None]
    dead4 = np.broadcast_to(dead[:, :, None, :], image.shape)
    with np.errstate(all="ignore"):
        scaled = (image * gain[:, :, None, None]).astype(np.float32)          # one fp32 multiply, round to nearest even
        exact = np.where(unit, image, scaled)
        exact = np.where(dead4, np.float32(0.0), exact).astype(np.float32)
        noisy = np.zeros(image.shape, bool)
        out = exact.astype(np.float64)
        bound = np.zeros(image.shape)
        if sigma > 0:
            noisy = ~dead4 & (np.ones(image.shape, bool) if noise_all else (image != 0))     # NaN != 0: lit
            z = normals(seed, seq, B, P, H, W)
            y = image.astype(np.float64) * gain.astype(np.float64)[:, :, None, None]
            s = float(sigma) * z
            full = np.where(np.isfinite(exact), y + s, exact.astype(np.float64))          # an fp32 product that overflowed stays what it is
            lim = C_ACC * U32 * ((Z_REL + 1.0) * np.abs(s) + np.where(unit, 0.0, np.abs(y)) + np.abs(full)) + FLOOR
            out = np.where(noisy, full, out)
            bound = np.where(noisy & np.isfinite(full), lim, 0.0)
    dead_all = dead.all(axis=1)                                               # [B, W]
    where = np.broadcast_to(dead_all[:, None, :], (B, H, W))
    lab = None if label is None else np.array(label, dtype=np.int64, copy=True)
    wgt = None if weight is None else np.array(weight, dtype=np.float32, copy=True)
    if lab is not None and dead_label is not None:
        lab[where] = dead_label
    if wgt is not None and dead_weight is not None:
        wgt[where] = np.float32(dead_weight)
    return dict(exact=exact, noisy=noisy, out=out, bound=bound, label=lab, weight=wgt, dead_all=dead_all)


def bound(x, gain, sigma, z):
    """the bound of one noisy element from scalars: x, gain, sigma the fp32 numbers, z the float64 normal"""
    x, gain, sigma = float(np.float32(x)), np.float32(gain), float(np.float32(sigma))
    unit = int(gain.view(np.uint32)) == ONE_BITS
    y, s = x * float(gain), sigma * float(z)
    return C_ACC * U32 * ((Z_REL + 1.0) * abs(s) + (0.0 if unit else abs(y)) + abs(y + s)) + FLOOR


def compare(got, ref):
    """got fp32 [B, P, H, W] against reference(): bit for bit where not noisy, within the bound where noisy (a NaN for a NaN, an
    infinity for itself) -> the worst ratio of an error to its bound"""
    got = np.ascontiguousarray(got, dtype=np.float32).reshape(ref["exact"].shape)
    quiet = ~ref["noisy"]
    bad = quiet & (got.view(np.int32) != ref["exact"].view(np.int32))
    assert not bad.any(), "%d elements without noise differ in their bits, first at %s" % (bad.sum(), tuple(np.argwhere(bad)[0]))
    out, lim = ref["out"], ref["bound"]
    with np.errstate(all="ignore"):
        wild = ref["noisy"] & ~np.isfinite(out)
        same = np.where(np.isnan(out), np.isnan(got), got.astype(np.float64) == out)
        assert same[wild].all(), "a NaN or an infinity under noise did not stay what it was"
        live = ref["noisy"] & ~wild
        err = np.abs(got.astype(np.float64) - out)
    if not live.any():
        return 0.0
    ratio = err[live] / lim[live]
    worst = float(ratio.max())
    assert worst <= 1.0, "a noisy element is %.3f bounds from the float64 reference (error %.3e, bound %.3e)" % (
        worst, err[live][ratio.argmax()], lim[live][ratio.argmax()])
    return worst


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
def crop(rs, B, P, H, W, lit=0.1):
    """a thresholded crop: zeros with a share `lit` of pixels in [10, 200)"""
    x = rs.uniform(10.0, 200.0, (B, P, H, W)).astype(np.float32)
    x[rs.rand(B, P, H, W) >= lit] = 0.0
    return x
