"""ctypes binding of libubresnet_dice.so (the C ABI in include/ubresnet_dice.h): the soft Dice / Tversky region loss on the device
-- a streaming pass that leaves one row of per-class partial sums per workgroup, one workgroup that adds them in a fixed order
into a control block and derives two coefficients per class, and the backward that multiplies with those coefficients.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch, so the argument checks of the library can be exercised on a machine
without a GPU.
"""
from __future__ import annotations

import ctypes as C
import struct

from ._binding import Binding

BLOCK = 256          # UBK_BLOCK
UNROLL = 2           # UBK_UNROLL
MAX_GRID = 1024      # UBK_MAX_GRID
MAX_CLASSES = 16     # UBK_MAX_CLASSES
REG_CLASSES = 4      # UBK_REG_CLASSES
TRIP_PIXELS = BLOCK * UNROLL * 4
ROW_WORDS = 66       # UBK_ROW_WORDS
WORKSPACE_BYTES = MAX_GRID * ROW_WORDS * 8
CTL_WORDS = 116      # UBK_CTL_WORDS
CTL_BYTES = CTL_WORDS * 8
# the words of the control block (UBK_CTL_*)
CTL = dict(TP=0, FP=16, FN=32, PIXELS=48, VALID=64, BAD=65, T=66, K1=82, K0=98, S=114, LOSS=115)
# the words of a workspace row (UBK_ROW_*)
ROW = dict(TP=0, FP=16, FN=32, PIXELS=48, VALID=64, BAD=65)

vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float
BINDING = Binding("UBK_LIB", "libubresnet_dice.so", "ubk", {
    "ubk_dice_fwd": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i64, f32, f32, f32, i32, vp, vp, vp, vp]),
    "ubk_dice_bwd": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i64, vp, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


def grid(pixels: int) -> int:
    """workgroups (= workspace rows) of the streaming passes over `pixels` = N*H*W"""
    return min((int(pixels) + TRIP_PIXELS - 1) // TRIP_PIXELS, MAX_GRID)


def dice_fwd(predict: int, target: int, pixelweights: int, classw, N, Cn, H, W, ignore_index, alpha, beta, eps, present_only,
             workspace: int, ctl: int, loss: int, stream=None):
    """ubk_dice_fwd on raw device addresses (classw: an address or None)"""
    check(lib().ubk_dice_fwd(predict, target, pixelweights, classw, int(N), int(Cn), int(H), int(W), int(ignore_index), float(alpha),
                             float(beta), float(eps), int(bool(present_only)), workspace, ctl, loss, stream), "dice_fwd")


def dice_bwd(g_loss: int, ctl: int, predict: int, target: int, pixelweights: int, N, Cn, H, W, ignore_index, g_predict: int, stream=None):
    """ubk_dice_bwd on raw device addresses"""
    check(lib().ubk_dice_bwd(g_loss, ctl, predict, target, pixelweights, int(N), int(Cn), int(H), int(W), int(ignore_index), g_predict,
                             stream), "dice_bwd")


def read_ctl(raw: bytes) -> dict:
    """the control block (CTL_BYTES bytes, as copied to the host) as a dict of Python numbers and lists of MAX_CLASSES"""
    assert len(raw) >= CTL_BYTES
    f64 = struct.unpack_from("<%dd" % CTL_WORDS, raw)
    u64 = struct.unpack_from("<%dQ" % CTL_WORDS, raw)
    f32w = struct.unpack_from("<%df" % (2 * CTL_WORDS), raw)

    def per_class(words, at):
        return list(words[CTL[at]:CTL[at] + MAX_CLASSES])
    return dict(tp=per_class(f64, "TP"), fp=per_class(f64, "FP"), fn=per_class(f64, "FN"), pixels=per_class(u64, "PIXELS"),
                valid=u64[CTL["VALID"]], bad=u64[CTL["BAD"]], T=per_class(f64, "T"),
                k1=[f32w[2 * (CTL["K1"] + c)] for c in range(MAX_CLASSES)], k0=[f32w[2 * (CTL["K0"] + c)] for c in range(MAX_CLASSES)],
                S=f64[CTL["S"]], loss=f32w[2 * CTL["LOSS"]])
