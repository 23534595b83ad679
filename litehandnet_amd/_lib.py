"""ctypes binding of liblhn.so -- the C ABI declared in include/lhn.h.

There is no CPU fallback: if the shared library is missing or no gfx950 device is usable the
product path raises.  (The CPU oracle lives in /oracle and is test infrastructure only.)
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblhn.so")
_lib = None


class LhnError(RuntimeError):
    pass


class View(C.Structure):
    _fields_ = [("data", C.c_void_p), ("table", C.c_void_p), ("gate", C.c_void_p),
                ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("cstride", C.c_int32), ("coff", C.c_int32), ("C", C.c_int32), ("pend", C.c_void_p)]


class GradView(C.Structure):
    _fields_ = [("dz", C.c_void_p), ("dpool", C.c_void_p), ("coef", C.c_void_p)]


class CcwSe(C.Structure):
    """lhn_ccw_se: SpatialWeighting's parameters of one branch (lhn_ccw_shuffle_fwd)."""
    _fields_ = [("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p), ("J", C.c_int32)]


class Op(C.Structure):
    _fields_ = [("kind", C.c_int32),
                ("in_buf", C.c_int32 * 3), ("in_coff", C.c_int32 * 3), ("in_C", C.c_int32 * 3), ("reserved", C.c_int32 * 6),
                ("out_buf", C.c_int32), ("out_coff", C.c_int32), ("out_C", C.c_int32),
                ("p", C.c_int32 * 12), ("ws", C.c_int64 * 12), ("i", C.c_int32 * 8), ("f", C.c_float * 8)]


class Buf(C.Structure):
    _fields_ = [("data_off", C.c_int64), ("table_off", C.c_int64), ("gate_off", C.c_int64),
                ("grad_off", C.c_int64), ("dpool_off", C.c_int64), ("coef_off", C.c_int64),
                ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32)]


# every exported symbol of include/lhn.h (tests check the .so exports all of them)
SYMBOLS = [
    "lhn_version", "lhn_deterministic", "lhn_last_error", "lhn_device_ok",
    "lhn_heatmap_encode", "lhn_heatmap_argmax", "lhn_heatmap_refine", "lhn_transform_preds",
    "lhn_heatmap_decode", "lhn_heatmap_decode_dark", "lhn_heatmap_decode_dark_udp", "lhn_heatmap_nms", "lhn_heatmap_topk", "lhn_pck_accuracy",
    "lhn_eval_state_bytes", "lhn_eval_accumulate", "lhn_eval_finalize",
    "lhn_loss_balanced_mse_fwd", "lhn_loss_balanced_mse_bwd", "lhn_affine_warp_normalize", "lhn_affine_warp_normalize2", "lhn_random_flip", "lhn_hsv_jitter", "lhn_simdr_encode", "lhn_simdr_loss_fwd", "lhn_simdr_loss_bwd",
    "lhn_conv_pw_fwd", "lhn_conv_pw_fwd2", "lhn_conv_pw_bwd2", "lhn_conv_dw_fwd", "lhn_conv_dw_fwd2", "lhn_conv_dw_fwd3", "lhn_conv_pw_dw3_fwd", "lhn_conv_dw3_pw_fwd", "lhn_msrb_round_scratch_bytes", "lhn_msrb_round_fwd", "lhn_bottleneck_fwd", "lhn_stem_tail_fwd", "lhn_conv_stem_fwd", "lhn_conv_kxk_fwd", "lhn_conv_kxk_fwd_bf16x3",
    "lhn_bn_finalize", "lhn_table_fill", "lhn_table_bias", "lhn_fold_bn", "lhn_ew_fwd", "lhn_ew_fwd2", "lhn_ew_fwd3", "lhn_ew_mul_bwd", "lhn_bilinear_bwd", "lhn_shuffle2_fwd", "lhn_shuffle2_bwd", "lhn_bn_finalize2", "lhn_bn_bwd_finalize2", "lhn_maxpool2_fwd", "lhn_avgpool_fwd", "lhn_avgpool_fwd2", "lhn_avgpool_bwd2", "lhn_se_mlp_fwd2", "lhn_se_mlp_bwd2", "lhn_ca_mlp_fwd", "lhn_att_mlp_fwd", "lhn_att_mlp_bwd", "lhn_se_mlp_fwd", "lhn_se_mlp_bwd",
    "lhn_bn_bwd_reduce", "lhn_bn_bwd_finalize", "lhn_conv_pw_bwd", "lhn_conv_dw_bwd", "lhn_conv_dw_bwd2", "lhn_conv_dw_bwd3", "lhn_conv_dw_bwd4", "lhn_conv_dw_route", "lhn_conv_pw_route", "lhn_conv_kxk_route", "lhn_conv_pw_bwd4", "lhn_conv_pw_bwd5", "lhn_conv_pw_bwd6", "lhn_plan_head_gate_fold", "lhn_plan_pw_dz_dead", "lhn_plan_fwd_fin_consumer", "lhn_conv_dw_fwd4", "lhn_conv_pw_fwd3", "lhn_conv_stem_bwd",
    "lhn_conv_kxk_bwd", "lhn_ew_bwd", "lhn_ew_bwd2", "lhn_maxpool2_bwd", "lhn_maxpool2_bwd2", "lhn_maxpool2_bwd3", "lhn_ew_bwd3", "lhn_ew_bwd_multi", "lhn_avgpool_bwd3", "lhn_conv_pw_bwd3", "lhn_avgpool_bwd", "lhn_gate_bwd_reduce", "lhn_gate_bwd_reduce2", "lhn_gate_bwd_reduce3", "lhn_adam_step", "lhn_avgpool_fwd3", "lhn_avgpool_fwd4", "lhn_ca_mlp_bwd2",
    "lhn_ca_mlp_bwd", "lhn_reduce_replicas", "lhn_fold_stat_replicas", "lhn_plan_create", "lhn_plan_destroy", "lhn_plan_run", "lhn_plan_run_range",
    "lhn_cbam_layout", "lhn_cbam_fwd", "lhn_cbam_bwd",
    "lhn_ccw_scratch_bytes", "lhn_ccw_pool_fwd", "lhn_ccw_gate_fwd", "lhn_ccw_dw_fwd", "lhn_ccw_shuffle_fwd",
    "lhn_maxpool2_fwd_pair", "lhn_maxpool2_bwd_pair", "lhn_ew_fwd_pair", "lhn_ew_bwd_pair", "lhn_ew_bwd_multi_pair", "lhn_avgpool_fwd_pair",
    "lhn_bn_finalize_pair", "lhn_plan_pair",
]


def lib():
    """Load liblhn.so (once).  Raises LhnError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LhnError(f"{LIB_PATH} is missing: run `python -m litehandnet_amd.build` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        _lib = C.CDLL(LIB_PATH)
        _lib.lhn_last_error.restype = C.c_char_p
        _lib.lhn_plan_create.restype = C.c_void_p
        _lib.lhn_plan_destroy.restype = None
        _lib.lhn_eval_state_bytes.restype = C.c_int64
        # (backward, H, W, C, k, stride, pad, dil, features, switches) -> kernel name or NULL; host only
        _lib.lhn_conv_dw_route.argtypes = [C.c_int] * 10
        _lib.lhn_conv_dw_route.restype = C.c_char_p
        # (backward, N, H, W, Cin, Cout, stride, w_rows, w_cols, features, switches) -> the launches in order or NULL; host only
        _lib.lhn_conv_pw_route.argtypes = [C.c_int] * 11
        _lib.lhn_conv_pw_route.restype = C.c_char_p
        # (backward, N, H, W, Cin, Cout, stride, nrep, features, cus, switches) -> the launches in order or NULL; host only
        _lib.lhn_conv_kxk_route.argtypes = [C.c_int] * 11
        _lib.lhn_conv_kxk_route.restype = C.c_char_p
        # (x, w_dw, dil, t_table, w_pw, bias, y, stream)
        _lib.lhn_conv_dw3_pw_fwd.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.lhn_conv_dw3_pw_fwd.restype = C.c_int
        _lib.lhn_msrb_round_scratch_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
        _lib.lhn_msrb_round_scratch_bytes.restype = C.c_int64
        # (x[2], extra[2] or NULL, coef2, w_d1, w_d2, y, pooled, OH, OW, scratch, stream)
        _lib.lhn_msrb_round_fwd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                            C.c_void_p, C.c_void_p]
        _lib.lhn_msrb_round_fwd.restype = C.c_int
        # (x, Cm, w1, b1, t1, w2, t2, w3, b3, t3, out_slope, y, wt_scratch, stream)
        _lib.lhn_bottleneck_fwd.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.lhn_bottleneck_fwd.restype = C.c_int
        # (x, K, w_dw, bT, tT, w1, b1, tU, w2, b2, tV, w3, b3, y, wt_scratch, stream)
        _lib.lhn_stem_tail_fwd.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 14
        _lib.lhn_stem_tail_fwd.restype = C.c_int
        # (x, w, y, wsplit, relay, stream)
        _lib.lhn_conv_kxk_fwd_bf16x3.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib.lhn_conv_kxk_fwd_bf16x3.restype = C.c_int
        # (N, B, H[B], W[B], C[B]) -> bytes, 0 = unsupported; host only
        _lib.lhn_ccw_scratch_bytes.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.lhn_ccw_scratch_bytes.restype = C.c_int64
        # (x2[B], B, pooled, stream)
        _lib.lhn_ccw_pool_fwd.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _lib.lhn_ccw_pool_fwd.restype = C.c_int
        # (pooled, npix, Ct, mid, w1, t1, t1_stride, w2, t2, t2_stride, g, stream)
        _lib.lhn_ccw_gate_fwd.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_void_p]
        _lib.lhn_ccw_gate_fwd.restype = C.c_int
        # (x2[B], B, g, w[B], y[B], scratch, stream)
        _lib.lhn_ccw_dw_fwd.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        _lib.lhn_ccw_dw_fwd.restype = C.c_int
        # (x1[B], y[B], B, se[B], scratch, out[B], stream)
        _lib.lhn_ccw_shuffle_fwd.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4
        _lib.lhn_ccw_shuffle_fwd.restype = C.c_int
        _lib.lhn_cbam_layout.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.lhn_cbam_layout.restype = C.c_int
        # (p, r, w1, w2, w7, out, save, stream)
        _lib.lhn_cbam_fwd.argtypes = [C.c_void_p] * 8
        _lib.lhn_cbam_fwd.restype = C.c_int
        # (p, r, w1, w2, w7, out, dout, dp, dr, dw1, dw2, dw7, save, scratch, stream)
        _lib.lhn_cbam_bwd.argtypes = [C.c_void_p] * 15
        _lib.lhn_cbam_bwd.restype = C.c_int
    return _lib


def cbam_layout(N, H, W, Cc):
    """(save offsets [10], scratch offsets [8]) of lhn_cbam_fwd / lhn_cbam_bwd in floats (include/lhn.h: lhn_cbam_layout)."""
    sv, sc = (C.c_int64 * 10)(), (C.c_int64 * 8)()
    check(lib().lhn_cbam_layout(N, H, W, Cc, sv, sc), "lhn_cbam_layout")
    return list(sv), list(sc)


def check(status, what=""):
    if status != 0:
        raise LhnError(f"{what}: status {status}: {lib().lhn_last_error().decode()}")


def require_device(t=None):
    if not torch.cuda.is_available():
        raise LhnError("no GPU visible: litehandnet_amd has no CPU fallback")
    if t is not None and not t.is_cuda:
        raise LhnError("tensor must live on the GPU (litehandnet_amd has no CPU fallback)")


def ptr(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def f32c(t, name="tensor"):
    """float32, contiguous, on device -- validated, not converted silently across devices."""
    require_device(t)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()
