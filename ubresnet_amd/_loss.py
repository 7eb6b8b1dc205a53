"""ctypes binding of libubresnet_loss.so (the C ABI in include/ubresnet_loss.h): the pixel-wise focal loss and its normalised
means on the device -- a streaming pass that leaves one row of partials per workgroup, one workgroup that adds them in a fixed
order into a control block, and the backward that reads the reciprocal of the denominator from that block.

A self-contained library with its own error string, loaded through ubresnet_amd/_binding.py.  NO fallback: a missing library or a
failed call is a RuntimeError.  Nothing here imports torch, so the argument checks of the library can be exercised on a machine
without a GPU.
"""
from __future__ import annotations

import ctypes as C
import struct

from ._binding import Binding

BLOCK = 256          # UBL_BLOCK
UNROLL = 2           # UBL_UNROLL
MAX_GRID = 1024      # UBL_MAX_GRID
MAX_CLASSES = 16     # UBL_MAX_CLASSES
TRIP_PIXELS = BLOCK * UNROLL * 4
ROW_WORDS = 36       # UBL_ROW_WORDS
WORKSPACE_BYTES = MAX_GRID * ROW_WORDS * 8
CTL_WORDS = 40       # UBL_CTL_WORDS
CTL_BYTES = CTL_WORDS * 8
MEAN_PIXELS, MEAN_VALID, MEAN_WEIGHTS = 0, 1, 2
MODES = {"pixels": MEAN_PIXELS, "valid": MEAN_VALID, "weights": MEAN_WEIGHTS}
# the words of the control block (UBL_CTL_*)
CTL = dict(LOSS_SUM=0, WEIGHT_SUM=1, VALID=2, BAD=3, DENOM=4, INV_DENOM=5, LOSS=6, MODE=7, CLASS_LOSS=8, CLASS_PIXELS=24)
# the words of a workspace row (UBL_ROW_*)
ROW = dict(LOSS_SUM=0, WEIGHT_SUM=1, VALID=2, BAD=3, CLASS_LOSS=4, CLASS_PIXELS=20)

vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float
BINDING = Binding("UBL_LIB", "libubresnet_loss.so", "ubl", {
    "ubl_focal_fwd": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i64, f32, i32, vp, vp, vp, vp]),
    "ubl_focal_bwd": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i64, f32, vp, vp]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


def grid(pixels: int) -> int:
    """workgroups (= workspace rows) of the streaming passes over `pixels` = N*H*W"""
    return min((int(pixels) + TRIP_PIXELS - 1) // TRIP_PIXELS, MAX_GRID)


def focal_fwd(predict: int, target: int, pixelweights: int, classw, N, Cn, H, W, ignore_index, gamma, mode, workspace: int,
              ctl: int, loss: int, stream=None):
    """ubl_focal_fwd on raw device addresses (classw: an address or None)"""
    check(lib().ubl_focal_fwd(predict, target, pixelweights, classw, int(N), int(Cn), int(H), int(W), int(ignore_index), float(gamma),
                              int(mode), workspace, ctl, loss, stream), "focal_fwd")


def focal_bwd(g_loss: int, ctl: int, predict: int, target: int, pixelweights: int, classw, N, Cn, H, W, ignore_index, gamma,
              g_predict: int, stream=None):
    """ubl_focal_bwd on raw device addresses"""
    check(lib().ubl_focal_bwd(g_loss, ctl, predict, target, pixelweights, classw, int(N), int(Cn), int(H), int(W), int(ignore_index),
                              float(gamma), g_predict, stream), "focal_bwd")


def read_ctl(raw: bytes) -> dict:
    """the control block (CTL_BYTES bytes, as copied to the host) as a dict of Python numbers and lists"""
    assert len(raw) >= CTL_BYTES
    f64 = struct.unpack_from("<%dd" % CTL_WORDS, raw)
    u64 = struct.unpack_from("<%dQ" % CTL_WORDS, raw)
    f32w = struct.unpack_from("<%df" % (2 * CTL_WORDS), raw)
    return dict(loss_sum=f64[CTL["LOSS_SUM"]], weight_sum=f64[CTL["WEIGHT_SUM"]], valid=u64[CTL["VALID"]], bad=u64[CTL["BAD"]],
                denom=f64[CTL["DENOM"]], inv_denom=f32w[2 * CTL["INV_DENOM"]], loss=f32w[2 * CTL["LOSS"]], mode=u64[CTL["MODE"]],
                class_loss=list(f64[CTL["CLASS_LOSS"]:CTL["CLASS_LOSS"] + MAX_CLASSES]),
                class_pixels=list(u64[CTL["CLASS_PIXELS"]:CTL["CLASS_PIXELS"] + MAX_CLASSES]))
