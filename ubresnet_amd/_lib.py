"""ctypes binding of libubresnet_hip.so (the C ABI in include/ubresnet_hip.h).

Loaded through ubresnet_amd/_binding.py.  There is deliberately NO fallback: if the shared library
is missing or a call fails, a RuntimeError is raised (callers in the reference catch ``Exception`` and break their loop,
training/train_ubresnet2018_wlarcv2.py:230-239, so errors must be exceptions, never aborts).
"""
from __future__ import annotations

import ctypes as C

import torch

from ._binding import Binding

F32, BF16, F16 = 0, 1, 2
MAX_TAPS = 64
MAX_TILES = 64       # UBR_MAX_TILES
STAT_SLOTS = 32      # UBR_STAT_SLOTS
RED_SLOTS = 8        # UBR_RED_SLOTS
_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}
_CPU = {F32: 4, BF16: 8, F16: 8}


def dtype_id(dt: torch.dtype) -> int:
    try:
        return _DT[dt]
    except KeyError:
        raise RuntimeError("ubresnet_amd: unsupported compute dtype %s" % dt)


def chans_per_unit(dt: torch.dtype) -> int:
    return _CPU[dtype_id(dt)]


class Tensor(C.Structure):
    _fields_ = [("p", C.c_void_p), ("sn", C.c_int64), ("sy", C.c_int64), ("sx", C.c_int64)]


class ChanAffine(C.Structure):
    _fields_ = [("sub", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p), ("lo", C.c_void_p)]


class ConvDesc(C.Structure):
    _fields_ = [
        ("dtype", C.c_int32),
        ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32),
        ("x", Tensor),
        ("xf", ChanAffine),
        ("w", C.c_void_p),
        ("Cout", C.c_int32), ("Cout_pad", C.c_int32),
        ("ntaps", C.c_int32),
        ("dy", C.c_int8 * MAX_TAPS), ("dx", C.c_int8 * MAX_TAPS),
        ("wt", C.c_uint8 * MAX_TAPS),
        ("S", C.c_int32), ("iy0", C.c_int32), ("ix0", C.c_int32),
        ("OH", C.c_int32), ("OW", C.c_int32),
        ("y", Tensor),
        ("addend", Tensor),
        ("bias", C.c_void_p),
        ("stats", C.c_void_p),
        ("epilogue", C.c_int32),
        ("tile_hint", C.c_int32),
        ("act", C.c_int32),
        ("pad_", C.c_int32),
        ("addend_mask", C.c_void_p),
        ("bnb_c", Tensor),
        ("bnb_mean", C.c_void_p), ("bnb_scale", C.c_void_p), ("bnb_shift", C.c_void_p), ("bnb_invstd", C.c_void_p),
        ("nphase", C.c_int32), ("phase_tap0", C.c_int32 * 4), ("phase_ntaps", C.c_int32 * 4), ("pad3_", C.c_int32),
        ("phase_yoff", C.c_int64 * 4), ("phase_aoff", C.c_int64 * 4),
        ("stats_slots", C.c_int32), ("pad2_", C.c_int32),
    ]


class AsppFrontDesc(C.Structure):
    """ubr_aspp_front_desc"""
    _fields_ = [
        ("dtype", C.c_int32),
        ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
        ("pad_", C.c_int32),
        ("x", Tensor),
        ("w", C.c_void_p),
        ("bias", C.c_void_p),
        ("y", Tensor),
    ]


class BnFwdFin(C.Structure):
    """ubr_bn_fwd_fin"""
    _fields_ = [
        ("stats", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
        ("running_mean", C.c_void_p), ("running_var", C.c_void_p), ("num_batches_tracked", C.c_void_p),
        ("momentum", C.c_float), ("eps", C.c_float),
        ("scale", C.c_void_p), ("shift", C.c_void_p), ("mean", C.c_void_p), ("invstd", C.c_void_p),
    ]


class Pix(C.Structure):
    """ubr_pix"""
    _fields_ = [("p", C.c_void_p), ("ps", C.c_int64)]


PASS_REDUCE, PASS_APPLY, PASS_APPLY_FIN, PASS_FROZEN = 0, 1, 2, 3      # UBR_PASS_*


class BnSite(C.Structure):
    """ubr_bn_site"""
    _fields_ = [
        ("scale", C.c_void_p), ("shift", C.c_void_p), ("mean", C.c_void_p), ("invstd", C.c_void_p),
        ("k1", C.c_void_p), ("k2", C.c_void_p),
        ("red", C.c_void_p),
        ("dgamma", C.c_void_p), ("dbeta", C.c_void_p),
    ]


class BnBwdDesc(C.Structure):
    """ubr_bn_bwd_desc"""
    _fields_ = [
        ("dtype", C.c_int32), ("pass_", C.c_int32), ("relu", C.c_int32), ("C", C.c_int32),
        ("npix", C.c_int64),
        ("count", C.c_double),
        ("ga", Pix), ("ga2", Pix), ("c", Pix), ("gc", Pix),
        ("bn", BnSite),
    ]


class BlockTailBwdDesc(C.Structure):
    """ubr_block_tail_bwd_desc"""
    _fields_ = [
        ("dtype", C.c_int32), ("pass_", C.c_int32), ("C", C.c_int32), ("pad_", C.c_int32),
        ("npix", C.c_int64),
        ("count", C.c_double),
        ("go", Pix), ("go2", Pix), ("out", Pix), ("c2", Pix), ("cb", Pix), ("g_c2", Pix), ("g_sc", Pix),
        ("relu_mask", C.c_void_p),
        ("bn2", BnSite), ("bnb", BnSite),
    ]


class BlockTailFwdDesc(C.Structure):
    """ubr_block_tail_fwd_desc"""
    _fields_ = [
        ("dtype", C.c_int32), ("C", C.c_int32),
        ("npix", C.c_int64),
        ("count", C.c_double),
        ("c2", Pix), ("sc", Pix), ("out", Pix),
        ("relu_mask", C.c_void_p),
        ("mean2", C.c_void_p), ("scale2", C.c_void_p), ("shift2", C.c_void_p),
        ("mean_b", C.c_void_p), ("scale_b", C.c_void_p), ("shift_b", C.c_void_p),
        ("fin2", C.POINTER(BnFwdFin)), ("fin_b", C.POINTER(BnFwdFin)),
    ]


REDUCE_BATCH = 16         # UBR_REDUCE_BATCH


class WgradReduceItem(C.Structure):
    _fields_ = [
        ("slabs", C.c_void_p), ("dst", C.c_void_p),
        ("nsplit", C.c_int32), ("ntaps", C.c_int32), ("Cout_pad", C.c_int32), ("Cin", C.c_int32),
        ("Cout_valid", C.c_int32), ("Cin_valid", C.c_int32), ("accumulate", C.c_int32), ("pad_", C.c_int32),
        ("sm", C.c_int64), ("sk", C.c_int64),
        ("tapidx", C.c_int32 * 64),
    ]


class WgradDesc(C.Structure):
    _fields_ = [
        ("dtype", C.c_int32),
        ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32),
        ("x", Tensor),
        ("xf", ChanAffine),
        ("GH", C.c_int32), ("GW", C.c_int32), ("Cout", C.c_int32),
        ("g", Tensor),
        ("ntaps", C.c_int32),
        ("dy", C.c_int8 * MAX_TAPS), ("dx", C.c_int8 * MAX_TAPS),
        ("S", C.c_int32), ("iy0", C.c_int32), ("ix0", C.c_int32),
        ("slabs", C.c_void_p),
        ("nsplit", C.c_int32),
        ("exclusive", C.c_int32),
    ]


vp, i32, i64, f32, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double
I, P = C.c_int, C.POINTER
# every symbol include/ubresnet_hip.h declares, with its signature (tests check that all of them are exported)
BINDING = Binding("UBR_LIB", "libubresnet_hip.so", "ubr", {     # UBR_LIB: A/B builds of the same ABI (tools)
    "ubr_conv": (I, [P(ConvDesc), vp]),
    "ubr_conv_last_config": (None, [P(C.c_int)] * 4),
    "ubr_conv_last_kernel": (I, [C.c_char_p, i32]),
    "ubr_pack_weights": (I, [i32, vp, vp, i32, i32, i32, i32, i64, i64, i32, P(C.c_int32), vp]),
    "ubr_pack_weights_batched": (I, [i32, vp, i32, vp]),
    "ubr_bn_fold_batched": (I, [vp, i32, vp]),
    "ubr_aspp_front": (I, [P(AsppFrontDesc), vp]),
    "ubr_wgrad_plan": (I, [P(WgradDesc), P(C.c_int32), P(C.c_int64)]),
    "ubr_wgrad": (I, [P(WgradDesc), vp]),
    "ubr_wgrad_last_config": (None, [P(C.c_int)] * 5),
    "ubr_wgrad_last_pc": (I, []),
    "ubr_wgrad_reduce": (I, [vp, i32, i32, i32, i32, i32, i32, vp, i64, i64, P(C.c_int32), i32, vp]),
    "ubr_wgrad_reduce_batched": (I, [P(WgradReduceItem), i32, vp]),
    "ubr_stem_forward": (I, [i32, vp, i32, i32, i32, i32, vp, vp, i32, Tensor, vp, vp]),
    "ubr_stem_wgrad": (I, [i32, vp, i32, i32, i32, i32, Tensor, i32, vp, i64, vp, vp, i32, vp]),
    "ubr_stem_wgrad_workspace": (i64, [i32] * 5),
    "ubr_stem_expand": (I, [i32, vp, i32, i32, i32, i32, vp, i64, vp]),
    "ubr_bn_finalize": (I, [vp, f64, vp, vp, vp, vp, vp, f32, f32, i32, vp, vp, vp, vp, vp]),
    "ubr_bn_eval_affine": (I, [vp, vp, vp, vp, f32, i32, vp, vp, vp, vp, vp]),
    "ubr_bn_bwd_finalize": (I, [vp, f64, i32, vp, vp, i32, vp, vp, vp]),
    "ubr_bn_bwd_finalize_frozen": (I, [vp, i32, vp, vp, vp, vp, vp]),
    "ubr_bn_bwd": (I, [P(BnBwdDesc), vp]),
    "ubr_block_tail_fwd": (I, [P(BlockTailFwdDesc), vp]),
    "ubr_block_tail_bwd": (I, [P(BlockTailBwdDesc), vp]),
    "ubr_maxpool_fwd": (I, [i32, i32, i32, i32, i32, i32, vp, i64, ChanAffine, vp, i64, vp, i64, vp, vp]),
    "ubr_maxpool_bwd": (I, [i32, i32, i32, i32, i32, i32, vp, i64, ChanAffine, vp, i64, vp, i64, vp, i64, vp, vp]),
    "ubr_logsoftmax_bwd": (I, [i32, i32, i32, i32, i32, vp, vp, vp, i64, vp]),
    "ubr_pixelwise_nll_fwd": (I, [vp, vp, vp, vp, i32, i32, i32, i32, i64, vp, vp, vp]),
    "ubr_pixelwise_nll_bwd": (I, [vp, vp, vp, vp, i32, i32, i32, i32, i64, vp, vp]),
    "ubr_confusion": (I, [vp, vp, i32, i32, i32, i32, vp, vp]),
    "ubr_channel_sum": (I, [i32, i64, i32, vp, i64, vp, vp]),
    "ubr_cast_f64_to_f32": (I, [vp, i32, i32, vp, i32, f64, i32, vp]),
    "ubr_zero": (I, [vp, i64, vp]),
    "ubr_adam_step": (I, [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, i64, f32, vp]),
    "ubr_sgd_step": (I, [vp, vp, vp, i64, f32, f32, f32, f32, i32, i32, f32, vp]),
    "ubr_crop_tiles": (I, [vp, i32, i32, i32, P(C.c_int32), i32, i32, i32, vp, vp]),
    "ubr_stitch_tiles": (I, [vp, i32, i32, i32, P(C.c_int32), i32, vp, i32, i32, i32, vp]),
    "ubr_last_error": (C.c_char_p, []),
    "ubr_version": (I, []),
    "ubr_tape_create": (vp, []),
    "ubr_tape_destroy": (None, [vp]),
    "ubr_tape_begin": (I, [vp, i32, P(vp)]),
    "ubr_tape_end": (I, [vp]),
    "ubr_tape_pause": (I, [vp, i32]),
    "ubr_tape_fork": (I, [vp, i32, i32]),
    "ubr_tape_mark": (I, [vp, i32]),
    "ubr_tape_wait_mark": (I, [vp, i32, vp]),
    "ubr_tape_size": (I, [vp]),
    "ubr_tape_replay": (I, [vp, i32, P(vp)]),
    "ubr_tape_set_label": (I, [vp, i32]),
    "ubr_tape_replay_timed": (I, [vp, i32, P(vp), P(C.c_float), P(C.c_int32), i32]),
    "ubr_launch_log": (I, [i32]),
    "ubr_launch_log_read": (I, [C.c_char_p, i32]),
})
LIB_PATH, SYMBOLS, lib, check = BINDING.path, BINDING.symbols, BINDING.lib, BINDING.check


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr() -> int:
    """raw hipStream_t of torch's current stream on the current device (every launch asks: the Python-level
    torch.cuda.current_stream() costs ~8 us per call, the raw query well under one)"""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def require_cuda(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError("ubresnet_amd: %s must live on a ROCm device (got %s); the HIP path has no CPU fallback"
                           % (what, t.device))


def ptr(t):
    return None if t is None else t.data_ptr()
