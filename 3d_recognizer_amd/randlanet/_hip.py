"""ctypes binding of librandla_hip.so (C ABI: include/rl_randlanet.h).

Nothing here touches HIP at import time (train.py spawns its worker with
multiprocessing 'spawn', reference train.py:108-115, so importing the package must not create
a GPU context).  The library is loaded on first use; if it is missing the product path fails
loudly - there is no CPU or PyTorch fallback for the kernels.
"""
import ctypes as C
import os
from typing import Optional

import torch

_LIB: Optional[C.CDLL] = None
_LIB_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc",
                         "librandla_hip.so")
# diagnostics only: an experimental build of the same library (kernel variants measured side by side, tools/pool_bench.py)
_LIB_PATH = os.environ.get("RL_HIP_LIB", _LIB_PATH)

ABI_VERSION = 110      # RL_VERSION the signatures below were written for (include/rl_randlanet.h; rounds 7 and 8 only append)
MAX_SLOTS = 1024
KNN_MAX_K = 64
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2

ERR_ARGS, ERR_FEW_SUPPORT, ERR_LAUNCH, ERR_UNSUPPORTED = -1, -2, -3, -4


class HipKernelError(RuntimeError):
    pass


class GemmDesc(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("lda", C.c_int64), ("a_bstride", C.c_int64),
        ("a_mode", C.c_int32), ("in_act", C.c_int32), ("in_slope", C.c_float),
        ("in_scale", C.c_void_p), ("in_shift", C.c_void_p),
        ("xyz", C.c_void_p), ("xyz_bstride", C.c_int64),
        ("nbr_idx", C.c_void_p), ("nbr_d2", C.c_void_p), ("nbr_k", C.c_int32),
        ("B", C.c_int32), ("n", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("W", C.c_void_p), ("w_ks", C.c_int64), ("w_ns", C.c_int64),
        ("bias", C.c_void_p),
        ("Y", C.c_void_p), ("ldy", C.c_int64), ("y_bstride", C.c_int64),
        ("accumulate", C.c_int32),
        ("stats", C.c_void_p),
        ("kslab", C.c_void_p), ("kslab_floats", C.c_int64),
        ("addend", C.c_void_p), ("out2", C.c_void_p), ("out2_index", C.c_void_p), ("out2_bstride", C.c_int64),
        ("split_col", C.c_int32),
        ("W_split", C.c_void_p),
        ("stats_pivot_mean", C.c_void_p), ("stats_pivot_bias", C.c_void_p),
        ("bnb_Y", C.c_void_p), ("bnb_scale", C.c_void_p), ("bnb_shift", C.c_void_p), ("bnb_mean", C.c_void_p),
        ("bnb_invstd", C.c_void_p), ("bnb_act", C.c_int32), ("bnb_slope", C.c_float),
        ("a2_split", C.c_int32), ("a2_act", C.c_int32), ("A2", C.c_void_p), ("lda2", C.c_int64), ("a2_bstride", C.c_int64),
        ("a2_idx", C.c_void_p), ("a2_scale", C.c_void_p), ("a2_shift", C.c_void_p), ("a2_slope", C.c_float),
        ("a2_first", C.c_int32),
    ]


class AttpoolSrc(C.Structure):
    _fields_ = [
        ("U", C.c_void_p), ("ldu", C.c_int64), ("u_scale", C.c_void_p), ("u_shift", C.c_void_p), ("u_act", C.c_int32),
        ("u_slope", C.c_float),
        ("G", C.c_void_p), ("ldg", C.c_int64), ("g_bstride", C.c_int64), ("g_scale", C.c_void_p), ("g_shift", C.c_void_p),
        ("g_act", C.c_int32), ("g_slope", C.c_float),
        ("idx", C.c_void_p), ("n", C.c_int32), ("h", C.c_int32),
    ]


class WsplitItem(C.Structure):
    _fields_ = [("W", C.c_void_p), ("w_ks", C.c_int64), ("w_ns", C.c_int64), ("K", C.c_int32), ("N", C.c_int32),
                ("out", C.c_void_p)]


class WgradDesc(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("lda", C.c_int64), ("a_bstride", C.c_int64),
        ("a_mode", C.c_int32), ("in_act", C.c_int32), ("in_slope", C.c_float),
        ("in_scale", C.c_void_p), ("in_shift", C.c_void_p),
        ("xyz", C.c_void_p), ("xyz_bstride", C.c_int64),
        ("nbr_idx", C.c_void_p), ("nbr_d2", C.c_void_p), ("nbr_k", C.c_int32),
        ("B", C.c_int32), ("n", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("dY", C.c_void_p), ("lddy", C.c_int64), ("dy_bstride", C.c_int64),
        ("dW", C.c_void_p), ("w_ks", C.c_int64), ("w_ns", C.c_int64),
        ("dbias", C.c_void_p),
        ("slab", C.c_void_p), ("slab_floats", C.c_int64),
        ("defer_reduce", C.c_int32), ("rows_bf16", C.c_int32),
        ("a2_split", C.c_int32), ("a2_act", C.c_int32), ("A2", C.c_void_p), ("lda2", C.c_int64), ("a2_bstride", C.c_int64),
        ("a2_idx", C.c_void_p), ("a2_scale", C.c_void_p), ("a2_shift", C.c_void_p), ("a2_slope", C.c_float),
        ("a2_first", C.c_int32),
    ]


class WgradReduceItem(C.Structure):
    _fields_ = [
        ("slab", C.c_void_p), ("dW", C.c_void_p), ("dbias", C.c_void_p),
        ("w_ks", C.c_int64), ("w_ns", C.c_int64),
        ("nsplit", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("reserved", C.c_int32),
    ]


class CloudJob(C.Structure):
    _fields_ = [
        ("xyz", C.c_void_p), ("features", C.c_void_p), ("labels", C.c_void_p), ("n_points", C.c_int64),
        ("xyz_f64", C.c_int32), ("normalization", C.c_int32), ("augment", C.c_int32), ("normal_col", C.c_int32),
        ("jitter_variance", C.c_double), ("jitter_limit", C.c_double), ("scale", C.c_double),
        ("R", C.c_double * 9), ("shift", C.c_double * 3),
    ]


class HeadDesc(C.Structure):
    _fields_ = [
        ("X", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p), ("act", C.c_int32), ("slope", C.c_float),
        ("mean", C.c_void_p), ("invstd", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p),
        ("perm", C.c_void_p), ("labels", C.c_void_p), ("B", C.c_int32), ("N", C.c_int32), ("C", C.c_int32),
        ("loss_kind", C.c_int32), ("alpha", C.c_float), ("gamma", C.c_float), ("neglect_background", C.c_int32),
        ("drop_p", C.c_float), ("drop_key", C.c_void_p), ("drop_seed", C.c_uint64), ("drop_first_row", C.c_int64),
        ("work", C.c_void_p), ("G", C.c_void_p), ("bn_bwd_stats", C.c_void_p), ("slab", C.c_void_p),
        ("slab_floats", C.c_int64), ("grad_scale", C.c_float), ("reserved", C.c_int32), ("drop_mask", C.c_void_p), ("perm_bstride", C.c_int64),
        ("class_weight", C.c_void_p), ("masked", C.c_int32),
    ]


class BnBwdDesc(C.Structure):
    _fields_ = [
        ("G", C.c_void_p), ("Y", C.c_void_p), ("ld", C.c_int64), ("bstride", C.c_int64),
        ("B", C.c_int32), ("n", C.c_int32), ("C", C.c_int32), ("act", C.c_int32),
        ("slope", C.c_float),
        ("scale", C.c_void_p), ("shift", C.c_void_p), ("mean", C.c_void_p), ("invstd", C.c_void_p),
        ("stats", C.c_void_p), ("coef", C.c_void_p),
    ]


class KnnTask(C.Structure):
    _fields_ = [
        ("support", C.c_void_p), ("support_bstride", C.c_int64), ("query", C.c_void_p), ("query_bstride", C.c_int64),
        ("Ns", C.c_int32), ("Nq", C.c_int32), ("k", C.c_int32),
        ("idx_out", C.c_void_p), ("d2_out", C.c_void_p),
    ]


KNN_MAX_TASKS = 8


class PoolDesc(C.Structure):
    _fields_ = [
        ("U", C.c_void_p), ("u_scale", C.c_void_p), ("u_shift", C.c_void_p), ("u_act", C.c_int32),
        ("u_slope", C.c_float),
        ("G", C.c_void_p), ("g_bstride", C.c_int64), ("g_scale", C.c_void_p), ("g_shift", C.c_void_p),
        ("g_act", C.c_int32), ("g_slope", C.c_float),
        ("idx", C.c_void_p), ("W", C.c_void_p), ("points", C.c_int64),
        ("n", C.c_int32), ("d", C.c_int32), ("nbr_k", C.c_int32),
        ("Pout", C.c_void_p), ("dP", C.c_void_p), ("GU", C.c_void_p), ("gu_accumulate", C.c_int32),
        ("DG", C.c_void_p), ("dW", C.c_void_p), ("slab", C.c_void_p), ("slab_floats", C.c_int64),
        ("X_out", C.c_void_p), ("dS_out", C.c_void_p),
        ("u_source", C.c_int32), ("xyz", C.c_void_p), ("xyz_bstride", C.c_int64), ("nbr_d2", C.c_void_p),
        ("W1", C.c_void_p), ("b1", C.c_void_p), ("scale1", C.c_void_p), ("shift1", C.c_void_p),
        ("W2", C.c_void_p), ("b2", C.c_void_p), ("scale2", C.c_void_p), ("shift2", C.c_void_p),
        ("mean1", C.c_void_p), ("invstd1", C.c_void_p), ("mean2", C.c_void_p), ("invstd2", C.c_void_p),
        ("xyz_width", C.c_int32), ("bn_bwd_stats", C.c_void_p), ("bn_fwd_stats2", C.c_void_p),
        ("rows_bf16", C.c_int32),
        ("pivot_mean1", C.c_void_p), ("pivot_mean2", C.c_void_p),
        ("x_optional", C.c_int32),
    ]


class ResidBnBwdDesc(C.Structure):
    _fields_ = [
        ("G", C.c_void_p), ("G2", C.c_void_p), ("O", C.c_void_p), ("slope", C.c_float), ("rows", C.c_int64), ("C", C.c_int32),
        ("Y1", C.c_void_p), ("scale1", C.c_void_p), ("mean1", C.c_void_p), ("invstd1", C.c_void_p),
        ("Y2", C.c_void_p), ("scale2", C.c_void_p), ("mean2", C.c_void_p), ("invstd2", C.c_void_p),
        ("stats1", C.c_void_p), ("stats2", C.c_void_p), ("coef1", C.c_void_p), ("coef2", C.c_void_p),
    ]


class CsrTask(C.Structure):
    _fields_ = [
        ("idx", C.c_void_p), ("n_src", C.c_int32), ("k", C.c_int32), ("n_dst", C.c_int32),
        ("offsets", C.c_void_p), ("entries", C.c_void_p),
    ]


CSR_MAX_TASKS = 8


class BnFinalizeItem(C.Structure):
    _fields_ = [
        ("stats", C.c_void_p), ("count", C.c_int64), ("gamma", C.c_void_p), ("beta", C.c_void_p),
        ("running_mean", C.c_void_p), ("running_var", C.c_void_p), ("num_batches_tracked", C.c_void_p),
        ("scale", C.c_void_p), ("shift", C.c_void_p), ("save_mean", C.c_void_p), ("save_invstd", C.c_void_p),
        ("folded_bias", C.c_void_p), ("nslots", C.c_int32), ("C", C.c_int32), ("training", C.c_int32),
        ("momentum", C.c_float), ("eps", C.c_float), ("pivoted", C.c_int32), ("pivot", C.c_void_p),
    ]


class BnBwdFinalizeItem(C.Structure):
    _fields_ = [
        ("stats", C.c_void_p), ("count", C.c_int64), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p), ("coef", C.c_void_p),
        ("nslots", C.c_int32), ("C", C.c_int32),
    ]


class SegsumDesc(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("lds", C.c_int64), ("src_bstride", C.c_int64),
        ("dst", C.c_void_p), ("ldd", C.c_int64), ("dst_bstride", C.c_int64),
        ("offsets", C.c_void_p), ("entries", C.c_void_p), ("entries_per_cloud", C.c_int64),
        ("B", C.c_int32), ("n_dst", C.c_int32), ("C", C.c_int32), ("accumulate", C.c_int32),
        ("src_bf16", C.c_int32),
    ]


class RowsDesc(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("lds", C.c_int64), ("src_bstride", C.c_int64),
        ("dst", C.c_void_p), ("ldd", C.c_int64),
        ("rows", C.c_int64), ("rows_per_batch", C.c_int64),
        ("C", C.c_int32),
        ("index32", C.c_void_p), ("index64", C.c_void_p),
        ("index_shared", C.c_int32), ("accumulate", C.c_int32), ("act", C.c_int32),
        ("slope", C.c_float),
        ("scale", C.c_void_p), ("shift", C.c_void_p),
    ]


_vp, _i, _l, _f, _d = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double
_SIGNATURES = {
    "rl_last_error": (C.c_char_p, []),
    "rl_last_kernel": (C.c_char_p, []),
    "rl_version": (_i, []),
    "rl_spin_us": (_i, [_i, _vp]),
    "rl_launch_count": (_l, []),
    "rl_row_blocks": (_i, [_l, _i]),
    "rl_knn_workspace_bytes": (_l, [_i, _i, _i, _i]),
    "rl_knn_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _l, _vp]),
    "rl_knn_f32_cpu": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "rl_knn_i32": (_i, [_vp, _l, _vp, _l, _i, _i, _i, _i, _vp, _vp, _vp, _l, _vp]),
    "rl_knn_multi_workspace_bytes": (_l, [C.POINTER(KnnTask), _i, _i]),
    "rl_knn_multi": (_i, [C.POINTER(KnnTask), _i, _i, _vp, _l, _vp]),
    "rl_gemm_streams": (_i, [C.POINTER(GemmDesc)]),
    "rl_gemm_pair_supported": (_i, [C.POINTER(GemmDesc), C.POINTER(GemmDesc)]),
    "rl_gemm_pair": (_i, [C.POINTER(GemmDesc), C.POINTER(GemmDesc), _vp]),
    "rl_gemm_kslab_floats": (_l, [_l, _i, _i]),
    "rl_gemm_stat_slots": (_l, [_l, _i, _i]),
    "rl_gemm": (_i, [C.POINTER(GemmDesc), _vp]),
    "rl_split_weights": (_i, [C.POINTER(WsplitItem), _i, _vp]),
    "rl_wgrad_slab_floats": (_l, [_l, _i, _i]),
    "rl_set_wide_gemm": (_i, [C.c_char_p]),
    "rl_get_wide_gemm": (C.c_char_p, []),
    "rl_set_wgemm_staging": (_i, [C.c_char_p]),
    "rl_set_wgemm_tile": (_i, [C.c_char_p]),
    "rl_set_gemm_ksplit": (_i, [_i]),
    "rl_set_sgemm_grid_div": (_i, [_i]),
    "rl_wgrad": (_i, [C.POINTER(WgradDesc), _vp]),
    "rl_wgrad_plan": (_i, [C.POINTER(WgradDesc), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_char_p)]),
    "rl_wgrad_plan2": (_i, [C.POINTER(WgradDesc), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_char_p),
                            C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_char_p)]),
    "rl_gemm_plan": (_i, [C.POINTER(GemmDesc), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                          C.POINTER(C.c_int32), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]),
    "rl_wgrad_nsplit": (_i, [_l, _i, _i]),
    "rl_wgrad_batchable": (_i, [C.POINTER(WgradDesc)]),
    "rl_wgrad_batch": (_i, [C.POINTER(WgradDesc), _i, _vp]),
    "rl_wgrad_reduce_batch": (_i, [C.POINTER(WgradReduceItem), _i, _vp]),
    "rl_bn_finalize": (_i, [_vp, _i, _l, _i, _vp, _vp, _vp, _vp, _vp, _f, _f, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "rl_bn_finalize_batch": (_i, [C.POINTER(BnFinalizeItem), _i, _vp]),
    "rl_bn_bwd_finalize_batch": (_i, [C.POINTER(BnBwdFinalizeItem), _i, _vp]),
    "rl_head_supported": (_i, [_i, _i]),
    "rl_head_grid": (_i, [_l]),
    "rl_head_fwd": (_i, [C.POINTER(HeadDesc), _vp, _vp]),
    "rl_head_bwd": (_i, [C.POINTER(HeadDesc), _vp]),
    "rl_bn_bwd_finalize_pair": (_i, [_vp, _vp, _i, _l, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rl_bn_reduce_slots": (_i, [_vp, _i, _i, _vp, _vp]),
    "rl_bn_bwd_slots": (_i, [_l]),
    "rl_bn_bwd_reduce": (_i, [C.POINTER(BnBwdDesc), _vp]),
    "rl_bn_bwd_finalize": (_i, [_vp, _i, _l, _i, _vp, _vp, _vp, _vp]),
    "rl_bn_bwd_apply": (_i, [C.POINTER(BnBwdDesc), _vp]),
    "rl_bn_bwd_fused_supported": (_i, [_l, _i, _l]),
    "rl_bn_bwd_fused": (_i, [C.POINTER(BnBwdDesc), _l, _vp, _vp, _vp, _vp]),
    "rl_resid_bn_bwd_supported": (_i, [_l, _i]),
    "rl_resid_bn_bwd_reduce": (_i, [C.POINTER(ResidBnBwdDesc), _vp]),
    "rl_resid_bn_bwd_apply": (_i, [C.POINTER(ResidBnBwdDesc), _vp]),
    "rl_resid_bn_bwd_fused_supported": (_i, [_l, _i]),
    "rl_resid_bn_bwd_fused": (_i, [C.POINTER(ResidBnBwdDesc), _vp, _vp, _vp, _vp, _vp]),
    "rl_copy_rows": (_i, [C.POINTER(RowsDesc), _vp]),
    "rl_copy_rows_pair": (_i, [C.POINTER(RowsDesc), C.POINTER(RowsDesc), _vp]),
    "rl_scatter_add_rows": (_i, [C.POINTER(RowsDesc), _vp]),
    "rl_csr_workspace_bytes": (_l, [C.POINTER(CsrTask), _i, _i]),
    "rl_csr_build": (_i, [C.POINTER(CsrTask), _i, _i, _vp, _l, _vp]),
    "rl_segment_sum_rows": (_i, [C.POINTER(SegsumDesc), _vp]),
    "rl_pool_supported": (_i, [_i, _i]),
    "rl_pool_slab_floats": (_l, [_l, _i]),
    "rl_pool_bwd_slots": (_i, [_l, _i]),
    "rl_pool_bwd_grid": (_i, [_l, _i, _i]),
    "rl_pool_fwd_slots": (_i, [_l, _i]),
    "rl_pool_fwd": (_i, [C.POINTER(PoolDesc), _vp]),
    "rl_rpe_stats_slots": (_i, [_l]),
    "rl_rpe_stats": (_i, [C.POINTER(PoolDesc), _vp, _vp]),
    "rl_rpe_bn_reduce": (_i, [C.POINTER(PoolDesc), _vp, _vp, _vp]),
    "rl_rpe_wgrad_slab_floats": (_l, [_l, _i, _i]),
    "rl_rpe_wgrad": (_i, [C.POINTER(PoolDesc), _vp, _vp, _vp, _l, _vp, _vp]),
    "rl_pool_bwd": (_i, [C.POINTER(PoolDesc), _vp]),
    "rl_set_pool128_x": (_i, [C.c_char_p]),
    "rl_get_pool128_x": (C.c_char_p, []),
    "rl_set_pool256_x": (_i, [C.c_char_p]),
    "rl_get_pool256_x": (C.c_char_p, []),
    "rl_set_decoder_cat": (_i, [C.c_char_p]),
    "rl_get_decoder_cat": (C.c_char_p, []),
    "rl_gemm_concat_supported": (_i, [C.POINTER(GemmDesc)]),
    "rl_attpool_cat_supported": (_i, [C.POINTER(AttpoolSrc), _l, _i, _i]),
    "rl_attpool_fwd_cat": (_i, [C.POINTER(AttpoolSrc), _vp, _l, _i, _i, _vp, _vp]),
    "rl_attpool_bwd_cat": (_i, [C.POINTER(AttpoolSrc), _vp, _vp, _vp, _l, _i, _i, _vp, _vp, _vp]),
    "rl_attpool_fwd": (_i, [_vp, _vp, _l, _i, _i, _vp, _vp]),
    "rl_attpool_bwd": (_i, [_vp, _vp, _vp, _vp, _l, _i, _i, _vp, _vp, _vp]),
    "rl_add_act_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _l, _i, _f, _vp, _vp]),
    "rl_add_act_bwd": (_i, [_vp, _vp, _l, _i, _f, _vp]),
    "rl_rpe_build": (_i, [_vp, _l, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "rl_rpe_build_dist": (_i, [_vp, _l, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "rl_batch_assemble": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rl_batch_assemble_scratch_doubles": (_l, [_i, _i]),
    "rl_batch_assemble_flag_u32": (_l, [_i, _i, _i]),
    "rl_batch_draw": (_i, [_vp, _i, _i, C.c_uint64, _vp, _vp, _vp]),
    "rl_scale_mask": (_i, [_vp, _vp, _f, _l, _vp]),
    "rl_dropout_tick": (_i, [_vp, _vp, _vp]),
    "rl_dropout_fwd": (_i, [_vp, _vp, _vp, _i, _f, _vp, _l, _l, _i, _vp, C.c_uint64, _f, _vp]),
    "rl_dropout_bwd": (_i, [_vp, _l, _l, _i, _vp, C.c_uint64, _f, _vp]),
    "rl_upsample_cf": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "rl_logits_unpermute": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "rl_logits_permute_grad": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "rl_logits_unpermute_b": (_i, [_vp, _vp, C.c_int64, _i, _i, _i, _vp, _vp]),
    "rl_logits_permute_grad_b": (_i, [_vp, _vp, C.c_int64, _i, _i, _i, _vp, _vp]),
    "rl_band_sort_workspace_bytes": (C.c_int64, [_i, _i, _vp, _i]),
    "rl_band_sort": (_i, [_vp, C.c_int64, _vp, _i, _i, _vp, _i, _vp, _vp, C.c_int64, _vp]),
    "rl_loss_max_classes": (_i, []),
    "rl_loss_work_doubles": (_l, [_l, _i]),
    "rl_loss_forward": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _f, _i, _vp, _vp, _vp]),
    "rl_loss_backward": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _f, _i, _vp, _f, _vp, _vp]),
    "rl_loss_forward_masked": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _f, _i, _vp, _i, _vp, _vp, _vp]),
    "rl_loss_backward_masked": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _f, _i, _vp, _f, _vp, _i, _vp, _vp]),
    "rl_loss_partials": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp, _vp]),
    "rl_loss_totals_offset": (_l, [_i]),
    "rl_loss_from_totals": (_i, [_l, _i, _i, _f, _f, _i, _vp, _vp, _vp]),
    "rl_loss_backward_global": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _f, _i, _vp, _f, _l, _vp, _vp]),
    "rl_lovasz_workspace_bytes": (_l, [_i, _i, _i]),
    "rl_lovasz_coef_offset": (_l, [_i, _i, _i]),
    "rl_lovasz_forward": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _l, _vp, _vp]),
    "rl_lovasz_backward": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _l, _f, _vp, _vp]),
    "rl_softmax_cf": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "rl_adam_step": (_i, [_vp, _vp, _vp, _vp, _l, _vp, _f, _f, _f, _f, _vp, _vp]),
    "rl_scene_workspace_bytes": (_l, [_l, _i]),
    "rl_scene_crop": (_i, [_vp, _l, _i, _vp, _i, _vp, _l, _vp, _vp, _l, _vp]),
    "rl_scene_accumulate": (_i, [_vp, _i, _i, _vp, _f, _f, _vp, _vp, _l, _vp]),
    "rl_scene_min_count": (_i, [_vp, _l, _vp, _vp, _vp]),
    "rl_scene_crop_padded": (_i, [_vp, _l, _i, _vp, _i, _vp, _l, _vp, _vp, _l, _vp]),
    "rl_scene_accumulate_first": (_i, [_vp, _i, _i, _vp, _f, _f, _vp, _vp, _l, _l, _i, _vp]),
    "rl_scenes_workspace_bytes": (_l, [_i, _l, _i]),
    "rl_scenes_init": (_i, [_vp, _i, _l, _vp, _vp, _l, _vp]),
    "rl_scenes_crop": (_i, [_vp, _i, _i, _l, _vp, _i, _i, _vp, _vp, _vp, _vp, _l, _vp]),
    "rl_scenes_crop_padded": (_i, [_vp, _i, _i, _l, _vp, _i, _i, _vp, _vp, _vp, _vp, _l, _vp]),
    "rl_scenes_vote_crop": (_i, [_vp, _i, _i, _l, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _l, _l, _vp, _vp, _vp, _vp, _vp, _l, _vp]),
    "rl_scenes_vote_accumulate": (_i, [_vp, _i, _i, _l, _l, _i, _vp, _vp, _f, _f, _vp, _l, _vp]),
    "rl_grid_workspace_bytes": (_l, [_l, _i]),
    "rl_grid_bounds": (_i, [_vp, _l, _i, _f, _vp, _vp, _l, _vp]),
    "rl_grid_sort": (_i, [_vp, _l, _i, _i, _vp, _l, _vp]),
    "rl_grid_heads": (_i, [_l, _i, _vp, _vp, _vp, _l, _vp]),
    "rl_grid_reduce": (_i, [_vp, _l, _i, _vp, _i, _l, _vp, _vp, _vp, _vp, _l, _vp]),
    "rl_scene_confusion": (_i, [_vp, _l, _i, _vp, _l, _vp, _vp, _vp]),
    "rl_cluster_workspace_bytes": (_l, [_l]),
    "rl_cluster_cells": (_i, [_vp, _l, _f, _vp, _vp, _l, _vp]),
    "rl_cluster_union": (_i, [_vp, _vp, _l, _f, _vp, _i, _i, _l, _vp, _vp, _vp, _l, _vp]),
    "rl_cluster_smooth_workspace_bytes": (_l, [_l]),
    "rl_cluster_union_smooth": (_i, [_vp, _vp, _l, _f, _vp, _i, _i, _l, _vp, _vp, _f, _f, _vp, _vp, _vp, _l, _vp]),
    "rl_cluster_dense_workspace_bytes": (_l, [_l, _i]),
    "rl_cluster_union_dense": (_i, [_vp, _vp, _l, _f, _vp, _i, _i, _l, _vp, _vp, _f, _f, _l, _vp, _vp, _vp, _l, _vp]),
    "rl_cluster_reduce": (_i, [_vp, _vp, _vp, _l, _l, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _vp]),
    "rl_scene_labels": (_i, [_vp, _l, _i, _f, _vp, _vp, _vp]),
    "rl_keypoints_workspace_bytes": (_l, [_l]),
    "rl_keypoints_cells": (_i, [_vp, _l, _f, _vp, _vp, _l, _vp]),
    "rl_keypoints_sort": (_i, [_vp, _vp, _vp, _l, _f, _vp, _i, _i, _vp, _l, _vp]),
    "rl_keypoints_support": (_i, [_vp, _l, _f, _vp, _l, _vp]),
    "rl_keypoints_peaks": (_i, [_vp, _l, _f, _l, _vp, _vp, _l, _vp]),
    "rl_keypoints_refine": (_i, [_vp, _l, _l, _f, _l, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _vp]),
    "rl_normals": (_i, [_vp, _l, _vp, _l, _l, _i, _vp, _vp, _vp, _vp, _vp]),
    "rl_pairs_workspace_bytes": (_l, [_l]),
    "rl_pairs_sort": (_i, [_vp, _i, _vp, _i, _l, _l, _l, _vp, _vp, _l, _vp]),
    "rl_pairs_write": (_i, [_l, _l, _l, _l, _vp, _vp, _vp, _vp, _l, _vp]),
    "rl_boxes_workspace_bytes": (_l, [_l, _l]),
    "rl_boxes_sort": (_i, [_vp, _i, _l, _l, _vp, _l, _vp]),
    "rl_boxes_moments": (_i, [_vp, _l, _l, _vp, _vp, _vp, _l, _vp]),
    "rl_boxes_fit": (_i, [_vp, _l, _l, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _vp]),
    "rl_outliers_workspace_bytes": (_l, [_l]),
    "rl_outliers_mean_distance": (_i, [_vp, _l, _l, _l, _i, _vp, _vp]),
    "rl_outliers_filter": (_i, [_vp, _l, _d, _vp, _vp, _vp, _vp, _vp, _l, _vp]),
    "rl_outliers_threshold": (_i, [_vp, _l, _d, _vp, _vp, _l, _vp]),
    "rl_outliers_compact": (_i, [_vp, _l, _vp, _vp, _vp, _vp, _vp, _l, _vp]),
    "rl_planes_workspace_bytes": (_l, [_l, _l]),
    "rl_planes_hypotheses": (_i, [_vp, _l, _vp, _l, _vp, _f, _vp, _vp, _vp]),
    "rl_planes_count": (_i, [_vp, _l, _vp, _l, _f, _vp, _vp, _vp, _l, _vp]),
    "rl_planes_split": (_i, [_vp, _l, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _l, _vp]),
    "rl_depth_workspace_bytes": (_l, [_l]),
    "rl_depth_points": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _f, _f, _f, _f, _vp, _f, _f, _i, _f, _f, _vp, _vp, _vp, _vp, _l, _vp]),
    "rl_icp_workspace_bytes": (_l, [_l]),
    "rl_icp_transform": (_i, [_vp, _l, _l, _l, C.POINTER(_f), _vp, _vp]),
    "rl_icp_sums": (_i, [_vp, _vp, _vp, _l, _vp, _vp, _l, _l, _l, _f, _i, _vp, _vp, _l, _vp]),
    "rl_icp_fold": (_i, [_l, _vp, _vp, _l, _vp]),
    "rl_fpfh_spfh": (_i, [_vp, _vp, _l, _vp, _vp, _l, _l, _i, _vp, _vp]),
    "rl_fpfh_fpfh": (_i, [_vp, _l, _vp, _vp, _l, _l, _i, _vp, _vp, _vp]),
    "rl_match_workspace_bytes": (_l, [_l, _l]),
    "rl_match_u8": (_i, [_vp, _l, _vp, _l, _vp, _vp, _vp, _l, _vp]),
    "rl_global_workspace_bytes": (_l, [_l, _l]),
    "rl_global_hypotheses": (_i, [_vp, _l, _vp, _l, _vp, _vp, _l, _f, _vp, _vp, _vp, _l, _vp]),
    "rl_global_count": (_i, [_vp, _l, _vp, _l, _vp, _vp, _l, _f, _vp, _vp, _l, _vp]),
    "rl_global_sums": (_i, [_vp, _l, _vp, _l, _vp, C.POINTER(_f), _f, _vp, _vp, _vp, _l, _vp]),
    "rl_tsdf_workspace_bytes": (_l, [_l]),
    "rl_tsdf_integrate": (_i, [_vp, _vp, _i, _i, _i, C.POINTER(_f), _f, _f, _i, _vp, _i, _i, _f, _f, _f, _f, _f, _f, _f,
                               C.POINTER(_f), _vp]),
    "rl_tsdf_count": (_i, [_vp, _vp, _i, _i, _i, C.POINTER(_f), _f, _i, _vp, _vp, _l, _vp]),
    "rl_tsdf_points": (_i, [_vp, _vp, _i, _i, _i, C.POINTER(_f), _f, _i, _l, _vp, _vp, _l, _vp, _l, _vp]),
}
EXPORTS = tuple(_SIGNATURES)
MAX_LOSS_CLASSES = 256       # RL_MAX_CLASSES of include/rl_randlanet.h (rl_loss_max_classes()): what every rl_loss_* entry takes


def library_path() -> str:
    return _LIB_PATH


def lib() -> C.CDLL:
    """Load librandla_hip.so (once).  Raises if it was not built - never falls back."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(_LIB_PATH):
            raise HipKernelError(
                f"{_LIB_PATH} not found: build it with `make -C 3d_recognizer_amd/csrc` "
                "(or __graft_entry__.build()); there is no fallback path for the HIP kernels")
        handle = C.CDLL(_LIB_PATH)
        handle.rl_version.restype = C.c_int
        have = handle.rl_version()
        if have != ABI_VERSION:      # a stale build (or an RL_HIP_LIB override from another revision): the argument lists differ
            raise HipKernelError(f"{_LIB_PATH} reports C-ABI version {have}, these bindings were written for {ABI_VERSION}: "
                                 "rebuild it (`make -C 3d_recognizer_amd/csrc`)")
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = handle
    return _LIB


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().rl_last_error().decode("utf-8", "replace")
        raise HipKernelError(f"{what or 'librandla_hip'} failed ({rc}): {msg}")


def gemm_plan(d: GemmDesc) -> dict:
    """What rl_gemm would launch for d (rl_gemm_plan; nothing is launched): {"rc"} for a refusal (rl_last_error says why), else
    also kernel, variant, grid, threads, tile (bm, bn), ksplit, reduce_cols."""
    grid, tile = (C.c_int32 * 3)(), (C.c_int32 * 2)()
    threads, ksplit, rcols = C.c_int32(), C.c_int32(), C.c_int32()
    kernel, variant = C.c_char_p(), C.c_char_p()
    rc = lib().rl_gemm_plan(C.byref(d), grid, C.byref(threads), tile, C.byref(ksplit), C.byref(rcols), C.byref(kernel), C.byref(variant))
    if rc != 0:
        return {"rc": rc}
    return {"rc": 0, "kernel": kernel.value.decode(), "variant": variant.value.decode(), "grid": tuple(grid), "threads": threads.value,
            "tile": tuple(tile), "ksplit": ksplit.value, "reduce_cols": rcols.value}


def wgrad_plan(d: WgradDesc) -> dict:
    """What rl_wgrad would launch for d (rl_wgrad_plan2; nothing is launched): {"rc"} for a refusal, else also kernel, variant, grid,
    threads, nsplit, rows_per_block, batch."""
    grid = (C.c_int32 * 3)()
    threads, nsplit, batch, rpb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    kernel, variant = C.c_char_p(), C.c_char_p()
    rc = lib().rl_wgrad_plan2(C.byref(d), grid, C.byref(threads), C.byref(kernel), C.byref(nsplit), C.byref(rpb), C.byref(batch),
                              C.byref(variant))
    if rc != 0:
        return {"rc": rc}
    return {"rc": 0, "kernel": kernel.value.decode(), "variant": variant.value.decode(), "grid": tuple(grid), "threads": threads.value,
            "nsplit": nsplit.value, "rows_per_block": rpb.value, "batch": batch.value}


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_GET_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def stream_ptr(device=None) -> int:
    """hipStream_t of torch's current stream as an integer.  The C-level accessors are used when torch has them:
    torch.cuda.current_stream() costs ~0.1 ms of Python per call (it re-checks torch.cuda.is_available() through
    os.environ every time), which was most of an eager forward's host time at ~130 launches."""
    if _RAW_STREAM is not None and _GET_DEVICE is not None and device is None:
        return _RAW_STREAM(_GET_DEVICE())
    return torch.cuda.current_stream(device).cuda_stream


def current_device() -> int:
    """Index of the current HIP device (the one whose current stream stream_ptr() returns)."""
    return _GET_DEVICE() if _GET_DEVICE is not None else torch.cuda.current_device()


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def row_blocks(rows: int, rows_per_tile: int) -> int:
    tiles = max(1, -(-rows // rows_per_tile))
    return min(tiles, MAX_SLOTS)
