"""Tensor-level wrappers over the C ABI (include/rl_randlanet.h).  PyTorch is used for device
memory and streams only; all arithmetic happens in librandla_hip.so.  Every wrapper checks
shapes on the host before launching (a faulting kernel can reset the GPU) and raises
HipKernelError on failure - there is no fallback implementation.
"""
import contextlib
import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _hip as H

F32 = torch.float32
BF16 = torch.bfloat16

# Storage of the neighbourhood-row tensors that only exist between two kernels of the backward pass (rl_randlanet.h
# "bf16-storage mode"): "f32" (default, the parity mode) or "bf16" - GU / DG of the fused pooling blocks and, on the
# 128-wide level, X / dS are then written and read as bf16 (half the bytes of the largest tensors of a step); coordinates,
# neighbour search, BatchNorm statistics, softmax, every accumulator, parameters and Adam stay fp32.
_STORAGE = os.environ.get("RL_STORAGE", "f32")


def set_storage(mode: str) -> None:
    global _STORAGE
    if mode not in ("f32", "bf16"):
        raise ValueError(f"storage must be 'f32' or 'bf16', got {mode!r}")
    if mode == "bf16" and get_wide_gemm() == "fp32":
        raise H.HipKernelError("bf16 storage needs the bf16x3 / bf16 arithmetic mode (RL_WIDE_GEMM)")
    _STORAGE = mode


def get_storage() -> str:
    return _STORAGE


def row_dtype() -> torch.dtype:
    """dtype of the (points*K)-row gradient tensors between backward kernels."""
    return BF16 if _STORAGE == "bf16" else F32


@dataclass
class Lazy:
    """A (rows, C) fp32 tensor whose value is act(raw*scale + shift) - the output of a
    SharedMLP before its BatchNorm+activation is applied (reference modules.py:93-104)."""
    raw: torch.Tensor                      # storage; logical rows are (B, n) with batch stride
    B: int
    n: int
    bstride: int                           # rows between clouds in `raw`
    C: int
    scale: Optional[torch.Tensor] = None
    shift: Optional[torch.Tensor] = None
    act: int = H.ACT_NONE
    slope: float = 0.0
    mean: Optional[torch.Tensor] = None    # saved batch statistics (training)
    invstd: Optional[torch.Tensor] = None
    bn: Optional[str] = None               # parameter prefix of its BatchNorm, if any

    @property
    def rows(self) -> int:
        return self.B * self.n

    def prefix(self, n: int) -> "Lazy":
        """First n rows of every cloud (the reference's random-sampling prefix slice)."""
        assert n <= self.n
        return Lazy(self.raw, self.B, n, self.bstride, self.C, self.scale, self.shift, self.act,
                    self.slope, self.mean, self.invstd, self.bn)


def plain(t: torch.Tensor, B: int, n: int) -> Lazy:
    assert t.dim() == 2 and t.shape[0] == B * n and t.is_contiguous()
    return Lazy(t, B, n, n, t.shape[1])


def _dev_check(*ts):
    """Every operand of a launch must be a contiguous tensor on the CURRENT HIP device: kernels go to the current
    device's current stream (H.stream_ptr), so a tensor living on another GPU would be dereferenced by the wrong
    device - a memory fault on a multi-GPU node.  Raised before anything is launched."""
    cur = H.current_device()
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise H.HipKernelError("HIP kernels need device tensors")
        if t.get_device() != cur:
            raise H.HipKernelError(
                f"tensor on cuda:{t.get_device()} but the current device is cuda:{cur}: run under "
                "`with torch.cuda.device(tensor.device)` (launches use the current device's stream)")
        if not t.is_contiguous():
            raise H.HipKernelError("HIP kernels need contiguous tensors")


def _st():
    return H.stream_ptr()


class KernelTimer:
    """Optional per-launch timing with HIP events on the launch stream (bench.py's roofline leg).
    Each record: (category, shape key, algorithmic bytes, flops, start event, end event)."""

    def __init__(self):
        self.records = []

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for cat, key, nbytes, flops, e0, e1, _kern, _lvl in self.records:
            a = agg.setdefault((cat, key), dict(category=cat, shape=key, launches=0, ms=0.0, bytes=0, flops=0))
            a["launches"] += 1
            a["ms"] += e0.elapsed_time(e1)
            a["bytes"] += nbytes
            a["flops"] += flops
        return sorted(agg.values(), key=lambda a: -a["ms"])


TIMER: Optional[KernelTimer] = None
LEVEL = -1      # encoder level the engine is working on (-1: outside the encoder) - a tag on the timer's records only


@contextlib.contextmanager
def level(l: int):
    """with level(l): <launches>  - the launches inside are filed under encoder level l by the timer."""
    global LEVEL
    keep, LEVEL = LEVEL, l
    try:
        yield
    finally:
        LEVEL = keep


NO_BN_SMALL = False      # test hook: small tensors take the three-launch BatchNorm path too
DEBUG_SYNC = bool(int(os.environ.get("RL_DEBUG_SYNC", "0")))   # print + sync around every launch


class _rec:
    """with _rec(category, key, bytes, flops): <one launch>  - free unless TIMER is set."""
    __slots__ = ("args", "e0")

    def __init__(self, cat, key, nbytes, flops=0):
        self.args = (cat, key, nbytes, flops)

    def __enter__(self):
        if DEBUG_SYNC:
            print("launch", self.args[0], self.args[1], flush=True)
        if TIMER is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if DEBUG_SYNC:
            torch.cuda.synchronize()
        if TIMER is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            kern = H.lib().rl_last_kernel().decode()
            TIMER.records.append(self.args + (self.e0, e1, kern, LEVEL))
        return False


# ------------------------------------------------------------------------------------- knn
def _knn_workspace(device, B: int, Ns: int, Nq: int, k: int, brute: bool):
    """Scratch for the grid search (None -> tiled brute force inside the library)."""
    if brute or k > H.KNN_MAX_K or Ns < k:
        return None, 0
    nbytes = H.lib().rl_knn_workspace_bytes(B, Ns, Nq, k)
    if nbytes <= 0:
        return None, 0
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def _query_chunks(M: int, chunk: int, multiple: int = 1):
    """[(first, Q), ...]: M queries in chunks of at most `chunk`, rounded down to a multiple of `multiple` (one at least)."""
    Qmax = min(max(int(chunk) // multiple, 1) * multiple, M)
    return [(first, min(Qmax, M - first)) for first in range(0, M, Qmax)]


def _knn_chunk(support: torch.Tensor, queries: torch.Tensor, Q: int, k: int, idx: torch.Tensor, d2: torch.Tensor, ws=None):
    """One rl_knn_f32 launch of a chunked search: the k nearest rows of support (Ns, 3) for the Q rows `queries` starts at,
    into the rows `idx` / `d2` start at.  ws: the (workspace, bytes) of _knn_workspace(device, 1, Ns, Q, k, False) when the
    caller keeps one, made here otherwise."""
    Ns = support.shape[0]
    ws, nbytes = _knn_workspace(support.device, 1, Ns, Q, k, False) if ws is None else ws
    with _rec("knn", (1, Ns, Q, k), 12 * (Ns + Q) + 12 * Q * k, 8 * Ns * Q):
        H.check(H.lib().rl_knn_f32(support.data_ptr(), queries.data_ptr(), 1, Ns, Q, k, idx.data_ptr(), d2.data_ptr(),
                                   H.ptr(ws), nbytes, _st()), "rl_knn_f32")


def knn_i32(support: torch.Tensor, query: torch.Tensor, Ns: int, Nq: int, k: int, brute: bool = False
            ) -> Tuple[torch.Tensor, torch.Tensor]:
    """support (B, >=Ns, 3), query (B, >=Nq, 3): searches the first Ns / Nq points of each cloud."""
    _dev_check(support, query)
    assert support.dtype == F32 and query.dtype == F32 and support.shape[-1] == 3 and query.shape[-1] == 3
    B = support.shape[0]
    assert query.shape[0] == B and support.shape[1] >= Ns and query.shape[1] >= Nq
    idx = torch.empty((B, Nq, k), dtype=torch.int32, device=support.device)
    d2 = torch.empty((B, Nq, k), dtype=F32, device=support.device)
    ws, nbytes = _knn_workspace(support.device, B, Ns, Nq, k, brute)
    with _rec("knn", (B, Ns, Nq, k), B * (12 * (Ns + Nq) + 8 * Nq * k), 8 * B * Ns * Nq):
        H.check(H.lib().rl_knn_i32(support.data_ptr(), support.shape[1], query.data_ptr(), query.shape[1],
                                   B, Ns, Nq, k, idx.data_ptr(), d2.data_ptr(), H.ptr(ws), nbytes, _st()),
                "rl_knn_i32")
    return idx, d2


def knn_multi(xyz: torch.Tensor, tasks):
    """Several prefix searches over the same (B, N, 3) clouds in one launch set: tasks is a list of
    (Ns, Nq, k) - support = first Ns points, queries = first Nq points of every cloud.
    Returns [(idx int32 (B,Nq,k), d2 fp32 (B,Nq,k)), ...]."""
    _dev_check(xyz)
    assert xyz.dtype == F32 and xyz.dim() == 3 and xyz.shape[2] == 3
    B, N, _ = xyz.shape
    out = []
    for c0 in range(0, len(tasks), H.KNN_MAX_TASKS):
        chunk = tasks[c0:c0 + H.KNN_MAX_TASKS]
        arr = (H.KnnTask * len(chunk))()
        res = []
        nbytes_io = 0
        for t, (Ns, Nq, k) in zip(arr, chunk):
            assert 0 < k <= Ns <= N and 0 < Nq <= N and k <= H.KNN_MAX_K
            idx = torch.empty((B, Nq, k), dtype=torch.int32, device=xyz.device)
            d2 = torch.empty((B, Nq, k), dtype=F32, device=xyz.device)
            t.support, t.support_bstride, t.query, t.query_bstride = xyz.data_ptr(), N, xyz.data_ptr(), N
            t.Ns, t.Nq, t.k, t.idx_out, t.d2_out = Ns, Nq, k, idx.data_ptr(), d2.data_ptr()
            res.append((idx, d2))
            nbytes_io += B * (12 * (Ns + Nq) + 8 * Nq * k)
        nbytes = H.lib().rl_knn_multi_workspace_bytes(arr, len(chunk), B)
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=xyz.device)
        with _rec("knn_multi", tuple(chunk), nbytes_io, sum(8 * B * a * b for a, b, _ in chunk)):
            H.check(H.lib().rl_knn_multi(arr, len(chunk), B, ws.data_ptr(), ws.numel(), _st()), "rl_knn_multi")
        out.extend(res)
    return out


def knn_f32(support: torch.Tensor, query: torch.Tensor, k: int, brute: bool = False
            ) -> Tuple[torch.Tensor, torch.Tensor]:
    _dev_check(support, query)
    B, Ns, _ = support.shape
    Nq = query.shape[1]
    idx = torch.empty((B, Nq, k), dtype=torch.int64, device=support.device)
    d2 = torch.empty((B, Nq, k), dtype=F32, device=support.device)
    ws, nbytes = _knn_workspace(support.device, B, Ns, Nq, k, brute)
    with _rec("knn", (B, Ns, Nq, k), B * (12 * (Ns + Nq) + 12 * Nq * k), 8 * B * Ns * Nq):
        H.check(H.lib().rl_knn_f32(support.data_ptr(), query.data_ptr(), B, Ns, Nq, k, idx.data_ptr(),
                                   d2.data_ptr(), H.ptr(ws), nbytes, _st()), "rl_knn_f32")
    return idx, d2


# ------------------------------------------------------------------------------------ gemm
@dataclass
class Rpe:
    """Relative-position-encoding A operand (reference modules.py:173-186), never materialised."""
    xyz: torch.Tensor      # (B, n_parent, 3)
    idx: torch.Tensor      # (B, n, K) int32
    d2: torch.Tensor       # (B, n, K) fp32
    B: int
    n: int
    K: int

    @property
    def rows(self) -> int:
        return self.B * self.n * self.K


def set_wide_gemm(mode: str) -> None:
    """Arithmetic of the wide GEMM / weight-gradient kernels: "bf16x3" (default), "fp32" or "bf16" (rl_set_wide_gemm)."""
    H.check(H.lib().rl_set_wide_gemm(mode.encode()), "rl_set_wide_gemm")


def get_wide_gemm() -> str:
    return H.lib().rl_get_wide_gemm().decode()


def set_wgemm_staging(how: str) -> None:
    """Operand staging of the wide GEMM in the bf16 modes: "registers" or "dma" (rl_set_wgemm_staging); same results."""
    H.check(H.lib().rl_set_wgemm_staging(how.encode()), "rl_set_wgemm_staging")


def set_wgemm_tile(how: str) -> None:
    """Output tile of the LDS-DMA wide GEMM: "auto" (64-row / 64-column tiles for launches with few rows) or "128"; same Y."""
    H.check(H.lib().rl_set_wgemm_tile(how.encode()), "rl_set_wgemm_tile")


def set_gemm_ksplit(enable: bool) -> None:
    """Diagnostics: the K split of wide products with few output tiles on / off (rl_set_gemm_ksplit)."""
    H.check(H.lib().rl_set_gemm_ksplit(int(bool(enable))), "rl_set_gemm_ksplit")


def rpe_build(a: "Rpe", distances: bool = False) -> Lazy:
    """The relative position encoding of every neighbourhood row, written out once (rows x 12 floats: 10 channels +
    2 of padding) so that mlp_rpe1's forward and weight gradient read a plain tensor (modules.py:173-186)."""
    _dev_check(a.xyz, a.idx, a.d2)
    assert a.idx.dtype == torch.int32 and a.idx.shape == (a.B, a.n, a.K) and a.d2.shape == a.idx.shape
    assert a.xyz.shape[0] == a.B and a.xyz.shape[1] >= a.n and a.xyz.shape[2] == 3
    out = torch.empty((a.rows, 12), dtype=F32, device=a.xyz.device)
    with _rec("rpe_build", (a.rows,), (48 + 8) * a.rows, 0):
        fn = H.lib().rl_rpe_build_dist if distances else H.lib().rl_rpe_build     # a.d2 holds distances, not squares
        H.check(fn(a.xyz.data_ptr(), a.xyz.shape[1], a.idx.data_ptr(), a.d2.data_ptr(), a.B, a.n, a.K,
                   out.data_ptr(), _st()), "rl_rpe_build")
    return Lazy(out, a.B, a.n * a.K, a.n * a.K, 10)


@dataclass
class ConcatGather:
    """A (rows, u.C + g.C) operand that is never stored: row R of cloud b is [act(bn(u[R])) | act(bn(g[b, idx[R]]))] - the X of
    a pooling block, read where its halves live (rl_wgrad_desc.a2_*, rl_gemm_desc.a2_*, rl_attpool_src).  u: (B * n * 16) rows;
    g: the per-point table (any batch stride); idx (B, n, 16) int32, inside the cloud."""
    u: Lazy
    g: Lazy
    idx: torch.Tensor
    first = False          # column order [direct | gathered] (a2_first = 0)

    @property
    def B(self) -> int:
        return self.u.B

    @property
    def n(self) -> int:
        return self.u.n

    @property
    def C(self) -> int:
        return self.u.C + self.g.C

    @property
    def rows(self) -> int:
        return self.u.rows


@dataclass
class InterpConcat:
    """A decoder step's (rows, x.C + skip.C) concat that is never stored (modules.py:362): row R of cloud b is
    [act(bn(x[b, nn[R]])) | act(bn(skip[R]))] - the gathered half FIRST (a2_first = 1), one index per row.  x: the coarse level's
    output, a per-point table (any batch stride); skip: (B * n) dense rows; nn (B, n, 1) int32, inside the cloud."""
    x: Lazy
    skip: Lazy
    nn: torch.Tensor
    first = True

    # the two sources under the names the descriptor code reads (ConcatGather's): the direct rows, the table, the index
    @property
    def u(self) -> Lazy:
        return self.skip

    @property
    def g(self) -> Lazy:
        return self.x

    @property
    def idx(self) -> torch.Tensor:
        return self.nn

    @property
    def B(self) -> int:
        return self.skip.B

    @property
    def n(self) -> int:
        return self.skip.n

    @property
    def C(self) -> int:
        return self.x.C + self.skip.C

    @property
    def rows(self) -> int:
        return self.skip.rows


_CONCAT = (ConcatGather, InterpConcat)


def set_pool128_x(mode: str) -> None:
    """How the d = 128 pooling backward hands X to its weight gradient: "in_place" (X is not stored; the weight gradient reads
    U and the gathered rows of G) or "stored" (rl_set_pool128_x); same results."""
    H.check(H.lib().rl_set_pool128_x(mode.encode()), "rl_set_pool128_x")


def get_pool128_x() -> str:
    return H.lib().rl_get_pool128_x().decode()


def set_pool256_x(mode: str) -> None:
    """How the d = 256 pooling block (the un-fused path) hands X to its score product, attentive pooling and weight gradient:
    "in_place" (X is never stored; they read U and the gathered rows of G) or "stored" (rl_set_pool256_x); same results."""
    H.check(H.lib().rl_set_pool256_x(mode.encode()), "rl_set_pool256_x")


def get_pool256_x() -> str:
    return H.lib().rl_get_pool256_x().decode()


def set_decoder_cat(mode: str) -> None:
    """How a decoder step hands its concat [interpolated | skip] to its product and weight gradient: "in_place" (never stored;
    they read the coarse level's rows through the nearest-neighbour index and the skip tensor) or "stored"
    (rl_set_decoder_cat); same results."""
    H.check(H.lib().rl_set_decoder_cat(mode.encode()), "rl_set_decoder_cat")


def get_decoder_cat() -> str:
    return H.lib().rl_get_decoder_cat().decode()


def _fill_a(d, a):
    if isinstance(a, _CONCAT):
        u, g, idx = a.u, a.g, a.idx
        _dev_check(g.raw, g.scale, g.shift, idx)
        assert idx.dtype == torch.int32 and idx.numel() == u.rows and u.bstride == u.n and g.B == u.B
        assert g.raw.dtype == F32 and g.raw.dim() == 2 and g.raw.shape[1] >= g.C
        assert g.raw.shape[0] >= (g.B - 1) * g.bstride + g.n, "second source rows out of range"
        M, _ = _fill_a(d, u)
        d.K = u.C + g.C
        d.a2_split, d.A2, d.lda2, d.a2_bstride, d.a2_idx = u.C, g.raw.data_ptr(), g.raw.shape[1], g.bstride, idx.data_ptr()
        if a.first:
            d.a2_split, d.a2_first = g.C, 1
        if g.scale is not None:
            assert g.scale.numel() == g.C and g.shift.numel() == g.C
            d.a2_scale, d.a2_shift, d.a2_act, d.a2_slope = g.scale.data_ptr(), g.shift.data_ptr(), g.act, g.slope
        return M, u.C + g.C
    if isinstance(a, Rpe):
        _dev_check(a.xyz, a.idx, a.d2)
        assert a.idx.dtype == torch.int32 and a.idx.shape == (a.B, a.n, a.K) and a.d2.shape == a.idx.shape
        assert a.xyz.shape[0] == a.B and a.xyz.shape[1] >= a.n and a.xyz.shape[2] == 3
        d.a_mode = 1
        d.xyz, d.xyz_bstride = a.xyz.data_ptr(), a.xyz.shape[1]
        d.nbr_idx, d.nbr_d2, d.nbr_k = a.idx.data_ptr(), a.d2.data_ptr(), a.K
        d.B, d.n, d.K = a.B, a.n, 10
        return a.rows, 10
    _dev_check(a.raw, a.scale, a.shift)
    assert a.raw.dtype in (F32, BF16) and a.raw.dim() == 2 and a.raw.shape[1] >= a.C
    assert a.raw.shape[0] >= (a.B - 1) * a.bstride + a.n, "A operand rows out of range"
    d.a_mode = 0
    d.A, d.lda, d.a_bstride = a.raw.data_ptr(), a.raw.shape[1], a.bstride
    if a.scale is not None:
        assert a.scale.numel() == a.C and a.shift.numel() == a.C
        d.in_scale, d.in_shift, d.in_act, d.in_slope = a.scale.data_ptr(), a.shift.data_ptr(), a.act, a.slope
    d.B, d.n, d.K = a.B, a.n, a.C
    return a.rows, a.C


def weight_strides(W: torch.Tensor, transposed: bool, K: int, N: int) -> Tuple[int, int]:
    """(w_ks, w_ns) for a reference-layout weight: Conv2d/Linear (N,K[,1,1]) or
    ConvTranspose2d (K,N,1,1)."""
    if transposed:
        assert W.shape[0] == K and W.shape[1] == N, (tuple(W.shape), K, N)
        return N, 1
    assert W.shape[0] == N and W.shape[1] == K, (tuple(W.shape), K, N)
    return 1, K


# weights of the wide layers pre-split into bf16 head / tail planes, per orientation: split_weights() returns a dict
# (data_ptr, w_ks, w_ns, K, N) -> planes that the engine hands to gemm(wsplit=...) for the products of that pass only


def split_weights(entries) -> dict:
    """entries: list of (W, w_ks, w_ns, K, N[, True]).  One launch; returns {(data_ptr, w_ks, w_ns, K, N): planes}.  Products with
    N <= 64 and K <= 64 run on the streaming kernels and get no planes - unless the entry carries a sixth element (the narrow half of a
    gemm_pair)."""
    out_map = {}
    if get_wide_gemm() == "fp32" or not entries:
        return out_map
    entries = [e[:5] for e in entries if e[3] % 8 == 0 and (e[4] > 64 or e[3] > 64 or len(e) > 5)]
    if not entries:
        return out_map
    total = sum(2 * K * N + 8 for _, _, _, K, N in entries)
    buf = torch.empty(total, dtype=torch.bfloat16, device=entries[0][0].device)
    arr = (H.WsplitItem * len(entries))()
    off = 0
    for it, (W, ks, ns, K, N) in zip(arr, entries):
        _dev_check(W)
        assert W.dtype == F32 and W.numel() == K * N
        out = buf[off:off + 2 * K * N]
        it.W, it.w_ks, it.w_ns, it.K, it.N, it.out = W.data_ptr(), ks, ns, K, N, out.data_ptr()
        out_map[(W.data_ptr(), ks, ns, K, N)] = out
        off += (2 * K * N + 7) // 8 * 8           # 16-byte aligned planes
    with _rec("split_weights", (len(entries),), 6 * sum(K * N for _, _, _, K, N in entries), 0):
        H.check(H.lib().rl_split_weights(arr, len(entries), _st()), "rl_split_weights")
    return out_map


def gemm_stat_slots(M: int, N: int, K: int) -> int:
    """Slots of `stats` that gemm(..., stats=...) fills for an (M, K) x (K, N) product - the count bn_finalize must be given."""
    return int(H.lib().rl_gemm_stat_slots(M, N, K))


def gemm(a, W: torch.Tensor, w_ks: int, w_ns: int, N: int, bias: Optional[torch.Tensor] = None, *,
         out: Optional[torch.Tensor] = None, out_bstride: Optional[int] = None,
         accumulate: bool = False, stats: Optional[torch.Tensor] = None,
         addend: Optional[torch.Tensor] = None, out2: Optional[torch.Tensor] = None,
         out2_index: Optional[torch.Tensor] = None, out2_bstride: int = 0, split_col: int = 0,
         wsplit: Optional[dict] = None, pivot: Optional[tuple] = None, bnb: Optional[Lazy] = None, plan: Optional[dict] = None):
    """Y = A'.W (+ bias).  With `out2` (split epilogue, wide layers only): v = A'.W + addend; columns < split_col go to
    `out` (which then has split_col columns), the others to the dense (M, N - split_col) tensor `out2` (or, with
    `out2_index`, atomically to the rows it names) - the two halves of a concat's gradient in one pass.
    pivot (with stats): (running_mean, conv bias left out of this product or None) - the statistics are SHIFTED sums around
    running_mean - bias (rl_gemm_desc.stats_pivot_*); the matching bn_finalize call must say pivoted=True.
    bnb (a Lazy with batch statistics): this product is the complete gradient w.r.t. `bnb`'s ACTIVATED value and the streaming
    kernel takes it - the BatchNorm-backward sums of `bnb`'s layer come out as a by-product (rl_gemm_desc.bnb_*): returns
    (out, (partials, nslots)) with the pair bn_backward(stats=...) takes; (out, None) when the product does not qualify.
    plan (a dict, diagnostics): filled with rl_gemm_plan's answer for the very descriptor that is launched (H.gemm_plan)."""
    d = H.GemmDesc()
    M, K = _fill_a(d, a)
    cat = isinstance(a, _CONCAT)
    assert isinstance(a, Rpe) or (a.u.raw if cat else a.raw).dtype == F32, "rl_gemm reads fp32 rows"
    rows_per_batch = a.n * a.K if isinstance(a, Rpe) else a.n
    _dev_check(W, bias, out, stats)
    assert W.dtype == F32 and W.numel() == K * N
    if out is None:
        out = torch.empty((M, N), dtype=F32, device=W.device)
        out_bstride = rows_per_batch
    else:
        assert out.dtype == F32 and out.dim() == 2 and out.shape[1] >= (split_col if out2 is not None else N)
        out_bstride = rows_per_batch if out_bstride is None else out_bstride
        assert out.shape[0] >= (d.B - 1) * out_bstride + rows_per_batch, "Y rows out of range"
    if bias is not None:
        assert bias.numel() == N
    if stats is not None:
        assert stats.dtype == torch.float64 and stats.numel() >= gemm_stat_slots(M, N, K) * 2 * N
    d.N, d.W, d.w_ks, d.w_ns, d.bias = N, W.data_ptr(), w_ks, w_ns, H.ptr(bias)
    planes = wsplit.get((W.data_ptr(), w_ks, w_ns, K, N)) if wsplit else None
    if planes is not None:
        d.W_split = planes.data_ptr()
    d.Y, d.ldy, d.y_bstride, d.accumulate = out.data_ptr(), out.shape[1], out_bstride, int(accumulate)
    d.stats = H.ptr(stats)
    if pivot is not None:
        assert stats is not None and pivot[0].numel() == N and (pivot[1] is None or pivot[1].numel() == N)
        _dev_check(*pivot)
        d.stats_pivot_mean, d.stats_pivot_bias = pivot[0].data_ptr(), H.ptr(pivot[1])
    if addend is not None or out2 is not None:
        _dev_check(addend, out2, out2_index)
        assert addend is None or (addend.dtype == F32 and addend.shape == (M, N))
        if out2 is not None:
            assert out2.dtype == F32 and 0 < split_col < N and out2.shape[1] == N - split_col
            if out2_index is None:
                assert out2.shape[0] >= M
            else:
                assert out2_index.dtype == torch.int32 and out2_index.numel() == M
                assert out2.shape[0] >= (d.B - 1) * out2_bstride + 1
        d.addend, d.out2, d.out2_index = H.ptr(addend), H.ptr(out2), H.ptr(out2_index)
        d.out2_bstride, d.split_col = out2_bstride, split_col
    bnb_pre = None
    if bnb is not None:
        if (stats is None and pivot is None and bnb.mean is not None and bnb.scale is not None and bnb.raw.dtype == F32
                and bnb.raw.shape[1] == out.shape[1] and bnb.bstride == out_bstride and bnb.C == N
                and 4 * M * N <= BNB_MAX_BYTES and H.lib().rl_gemm_streams(C.byref(d))):
            _dev_check(bnb.raw, bnb.scale, bnb.shift, bnb.mean, bnb.invstd)
            st_b = new_stats(W.device, N)
            d.stats = st_b.data_ptr()
            d.bnb_Y, d.bnb_scale, d.bnb_shift = bnb.raw.data_ptr(), bnb.scale.data_ptr(), bnb.shift.data_ptr()
            d.bnb_mean, d.bnb_invstd, d.bnb_act, d.bnb_slope = bnb.mean.data_ptr(), bnb.invstd.data_ptr(), bnb.act, bnb.slope
            bnb_pre = (st_b, gemm_stat_slots(M, N, K))
    kfloats = H.lib().rl_gemm_kslab_floats(M, N, K) if (N > 64 and not isinstance(a, Rpe) and not cat and out2 is None and addend is None) else 0
    if kfloats > 0:
        kslab = _slab(W.device, kfloats)
        d.kslab, d.kslab_floats = kslab.data_ptr(), kslab.numel()
    if plan is not None:
        plan.update(H.gemm_plan(d))
    nbytes = 4 * (M * (K if not isinstance(a, Rpe) else 6) + M * N * (2 if accumulate else 1) + K * N)
    if cat:         # source 1 rows, the gathered table once (it stays in L2), one index per row; Y; W
        nbytes = 4 * (M * a.u.C + a.g.rows * a.g.C + M) + 4 * (M * N * (2 if accumulate else 1) + K * N)
    with _rec("gemm_rpe" if isinstance(a, Rpe) else "gemm", (M, K, N), nbytes, 2 * M * K * N):
        H.check(H.lib().rl_gemm(C.byref(d), _st()), "rl_gemm")
    return (out, bnb_pre) if bnb is not None else out


def gemm_concat_supported(a, W: torch.Tensor, w_ks: int, w_ns: int, N: int, wsplit: Optional[dict]) -> bool:
    """Does rl_gemm take this concat-gather operand for a plain product Y = A'.W under the process settings as they stand
    (rl_gemm_concat_supported: nothing is launched)?  rl_gemm_desc has no storage flag for the rows of a concat-gather operand -
    the kernel reads fp32 - so that one rule is answered here, from the tensors, before the library is asked."""
    if a.u.raw.dtype != F32 or a.g.raw.dtype != F32:
        return False
    d = H.GemmDesc()
    M, K = _fill_a(d, a)
    d.N, d.W, d.w_ks, d.w_ns = N, W.data_ptr(), w_ks, w_ns
    planes = wsplit.get((W.data_ptr(), w_ks, w_ns, K, N)) if wsplit else None
    if planes is not None:
        d.W_split = planes.data_ptr()
    d.Y, d.ldy, d.y_bstride = W.data_ptr(), N, a.n       # (a placeholder: the plan reads no memory)
    rc = H.lib().rl_gemm_concat_supported(C.byref(d))
    if rc not in (0, H.ERR_UNSUPPORTED):     # (a query, not a launch: only a malformed descriptor is reported)
        H.check(rc, "rl_gemm_concat_supported")
    return rc == 0


def gemm_split_supported(a: Lazy, W: torch.Tensor, w_ks: int, w_ns: int, N: int, split_col: int, wsplit: Optional[dict]) -> bool:
    """Does rl_gemm store this product in two pieces - columns below split_col to a (rows, split_col) tensor, the others to a dense
    (rows, N - split_col) one - under the process settings as they stand (the plan's answer: nothing is launched)?"""
    if a.raw.dtype != F32:
        return False
    d = H.GemmDesc()
    M, K = _fill_a(d, a)
    d.N, d.W, d.w_ks, d.w_ns = N, W.data_ptr(), w_ks, w_ns
    planes = wsplit.get((W.data_ptr(), w_ks, w_ns, K, N)) if wsplit else None
    if planes is not None:
        d.W_split = planes.data_ptr()
    d.Y, d.ldy, d.y_bstride = W.data_ptr(), split_col, a.n       # (placeholders: the plan reads no memory)
    d.out2, d.split_col = W.data_ptr(), split_col
    rc = H.lib().rl_gemm_concat_supported(C.byref(d))
    if rc not in (0, H.ERR_UNSUPPORTED):     # (a query, not a launch: only a malformed descriptor is reported)
        H.check(rc, "rl_gemm_concat_supported")
    return rc == 0


# the BatchNorm-backward sums as a by-product of the streaming input-gradient GEMM only for tensors up to this size: the epilogue
# reads the layer's output 4 bytes per lane, a reduce sweep 16 - on a large tensor that costs more than the launch it saves
# (fc_end.0 at 8 clouds: 84 MB, +13 us per step; measured)
BNB_MAX_BYTES = 32 << 20


def gemm_pair(a, first: tuple, second: tuple, wsplit: Optional[dict]):
    """Y1 = A'.W1 and Y2 = A'.W2 in ONE launch (rl_gemm_pair: mlp1 + shortcut of an encoder level, which share their input).
    first / second: (W, w_ks, w_ns, N, stats or None, pivot tuple or None).  Returns (Y1, Y2), or None when the pair cannot go out
    as one launch (the caller then issues two gemm() calls).  Statistics: H.row_blocks(M, 128) slots each."""
    if not wsplit or isinstance(a, Rpe) or a.raw.dtype != F32:
        return None
    descs, outs = [], []
    M = K = None
    for (W, w_ks, w_ns, N, stats, pivot) in (first, second):
        d = H.GemmDesc()
        M, K = _fill_a(d, a)
        planes = wsplit.get((W.data_ptr(), w_ks, w_ns, K, N))
        if planes is None:
            return None
        _dev_check(W, stats)
        out = torch.empty((M, N), dtype=F32, device=W.device)
        d.N, d.W, d.w_ks, d.w_ns, d.W_split = N, W.data_ptr(), w_ks, w_ns, planes.data_ptr()
        d.Y, d.ldy, d.y_bstride = out.data_ptr(), N, a.n
        if stats is not None:
            assert stats.dtype == torch.float64 and stats.numel() >= H.row_blocks(M, 128) * 2 * N
            d.stats = stats.data_ptr()
            if pivot is not None:
                _dev_check(*pivot)
                d.stats_pivot_mean, d.stats_pivot_bias = pivot[0].data_ptr(), H.ptr(pivot[1])
        descs.append(d)
        outs.append(out)
    if not H.lib().rl_gemm_pair_supported(C.byref(descs[0]), C.byref(descs[1])):
        return None
    N1, N2 = first[3], second[3]
    with _rec("gemm", (M, K, N1 + N2), 4 * (M * K + M * (N1 + N2) + K * (N1 + N2)), 2 * M * K * (N1 + N2)):
        H.check(H.lib().rl_gemm_pair(C.byref(descs[0]), C.byref(descs[1]), _st()), "rl_gemm_pair")
    return outs[0], outs[1]


_SLAB = {}


def _slab(device, floats: int) -> torch.Tensor:
    """Scratch for partial weight-gradient slabs: one growing buffer per (device, stream), reused in
    stream order (launches on one stream serialise, so consecutive users cannot overlap)."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    buf = _SLAB.get(key)
    if buf is None or buf.numel() < floats:
        buf = torch.empty(max(floats, 1 << 20), dtype=F32, device=device)
        _SLAB[key] = buf
    return buf


WGRAD_BATCH_BYTES = 3 << 30      # operands a queued group may pin


def wgrad(a, dY: torch.Tensor, dy_bstride: int, N: int, dW: torch.Tensor, w_ks: int, w_ns: int,
          dbias: Optional[torch.Tensor] = None, pending: Optional[list] = None, batch: Optional[list] = None,
          plan: Optional[dict] = None) -> None:
    """dW / dbias of a layer.  With `pending` (a list) only the per-workgroup partial slabs are produced, in a
    slab of their own, and the layer is queued for `wgrad_flush` - one reduction launch for a whole backward.
    With `batch` (a list, needs `pending`) a wide layer is not even launched here: its descriptor is queued for
    `wgrad_batch_flush`, which runs all of them as ONE grouped launch (they are independent of each other and small).
    plan (a dict, diagnostics): filled with rl_wgrad_plan2's answer for the very descriptor that is launched (H.wgrad_plan)."""
    d = H.WgradDesc()
    M, K = _fill_a(d, a)
    rows_per_batch = a.n * a.K if isinstance(a, Rpe) else a.n
    _dev_check(dY, dW, dbias)
    rows_bf16 = dY.dtype == BF16
    assert dY.dtype in (F32, BF16) and dY.dim() == 2 and dY.shape[1] >= N
    adt = F32 if isinstance(a, Rpe) else a.u.raw.dtype if isinstance(a, _CONCAT) else a.raw.dtype
    assert isinstance(a, Rpe) or adt == dY.dtype, "A and dY must share their storage type"
    d.rows_bf16 = int(rows_bf16)
    assert dY.shape[0] >= (d.B - 1) * dy_bstride + rows_per_batch
    assert dW.numel() == K * N and (dbias is None or dbias.numel() == N)
    floats = H.lib().rl_wgrad_slab_floats(M, N, K)
    slab = _slab(dY.device, floats) if pending is None else torch.empty(floats, dtype=F32, device=dY.device)
    d.N, d.dY, d.lddy, d.dy_bstride = N, dY.data_ptr(), dY.shape[1], dy_bstride
    d.dW, d.w_ks, d.w_ns, d.dbias = dW.data_ptr(), w_ks, w_ns, H.ptr(dbias)
    d.slab, d.slab_floats = slab.data_ptr(), slab.numel()
    d.defer_reduce = 0 if pending is None else 1
    es = 2 if rows_bf16 else 4
    nbytes, flops = es * (M * (K if not isinstance(a, Rpe) else 6) + M * N) + 4 * K * N, 2 * M * K * N
    if isinstance(a, _CONCAT):     # source 1 rows, the gathered table once (it stays in L2), one index per row; dY; dW
        nbytes = 4 * (M * a.u.C + a.g.rows * a.g.C + M) + 4 * M * N + 4 * K * N
    if plan is not None:
        plan.update(H.wgrad_plan(d))
    kind = H.lib().rl_wgrad_batchable(C.byref(d)) if (batch is not None and pending is not None) else 0
    if kind:
        # (the operands stay referenced by the queue entry until the grouped launch has been issued: the queue is flushed
        # early once it holds WGRAD_BATCH_BYTES of them, so that a large configuration does not keep every layer's A / dY
        # alive until the end of backward - a handful of grouped launches still remove most of the launch overhead)
        batch.append((d, nbytes, flops, a, dY, slab, kind))
        if sum(b[1] for b in batch) > WGRAD_BATCH_BYTES:
            wgrad_batch_flush(batch)
    else:
        with _rec("wgrad_rpe" if isinstance(a, Rpe) else "wgrad", (M, K, N), nbytes, flops):
            H.check(H.lib().rl_wgrad(C.byref(d), _st()), "rl_wgrad")
    if pending is not None:
        it = H.WgradReduceItem()
        it.slab, it.dW, it.dbias, it.w_ks, it.w_ns = slab.data_ptr(), dW.data_ptr(), H.ptr(dbias), w_ks, w_ns
        it.nsplit, it.N, it.K = H.lib().rl_wgrad_nsplit(M, N, K), N, K
        pending.append((it, slab, dW, dbias))


def wgrad_supported(a, dY: torch.Tensor, dy_bstride: int, N: int) -> bool:
    """Does rl_wgrad take this operand under the process settings as they stand (rl_wgrad_plan: nothing is launched)?"""
    d = H.WgradDesc()
    _fill_a(d, a)
    d.rows_bf16 = int(dY.dtype == BF16)
    d.N, d.dY, d.lddy, d.dy_bstride = N, dY.data_ptr(), dY.shape[1], dy_bstride
    d.dW = d.slab = dY.data_ptr()       # (placeholders: the plan reads no memory)
    d.slab_floats, d.defer_reduce = 1 << 62, 1
    rc = H.lib().rl_wgrad_plan(C.byref(d), None, None, None)
    if rc not in (0, H.ERR_UNSUPPORTED):     # (a query, not a launch: only a malformed descriptor is reported)
        H.check(rc, "rl_wgrad_plan")
    return rc == 0


def wgrad_batch_flush(batch: list) -> None:
    """The queued weight gradients as grouped launches (rl_wgrad_batch): one for the wide layers, one for the narrow
    (streaming) ones; before `wgrad_flush`."""
    for kind, name in ((1, "wgrad_batch"), (2, "swgrad_batch")):
        part = [b for b in batch if b[6] == kind]
        if not part:
            continue
        arr = (H.WgradDesc * len(part))(*[b[0] for b in part])
        with _rec(name, (len(part),), sum(b[1] for b in part), sum(b[2] for b in part)):
            H.check(H.lib().rl_wgrad_batch(arr, len(part), _st()), "rl_wgrad_batch")
    batch.clear()


def wgrad_flush(pending: list) -> None:
    """Sum the partial slabs of every queued layer (fixed order, deterministic) in one launch per 48 layers."""
    if not pending:
        return
    arr = (H.WgradReduceItem * len(pending))(*[p[0] for p in pending])
    nbytes = sum(4 * p[1].numel() for p in pending)
    with _rec("wgrad_reduce_batch", (len(pending),), nbytes, 0):
        H.check(H.lib().rl_wgrad_reduce_batch(arr, len(pending), _st()), "rl_wgrad_reduce_batch")
    pending.clear()


# -------------------------------------------------------------------------------------- bn
def new_stats(device, C: int) -> torch.Tensor:
    return torch.empty((H.MAX_SLOTS, 2, C), dtype=torch.float64, device=device)


class SyncGroup:
    """Data-parallel EQUIVALENCE mode: BatchNorm batch statistics and the loss' class sums are
    all-reduced over the ranks, so that N ranks on shards of a batch compute exactly the single-process step on the whole
    batch (up to fp32 summation order).  Not the throughput path: ~150 small collectives per step, no hipGraph.
    `staged=True` moves the (tiny, float64) records through host memory - for backends without device collectives
    (gloo rehearsals on a one-GPU box)."""

    def __init__(self, world: int, group=None, staged: bool = False):
        self.world, self.group, self.staged = world, group, staged
        # where this rank's shard sits in the global batch (set_shard); until then: `world` equal shards, rank unknown
        self.local_clouds, self.global_clouds, self.cloud_offset = 1, world, 0

    def set_shard(self, local_clouds: int, rank: Optional[int] = None) -> None:
        """Tell the group how many clouds this rank holds; the ranks exchange their counts (one tiny host all-reduce), so
        that shards of DIFFERENT sizes (a batch the world size does not divide) still normalise by the global row count
        and know their offset in the batch (Dropout mask slices)."""
        import torch.distributed as dist
        if self.world <= 1 or not (dist.is_available() and dist.is_initialized()):
            self.local_clouds, self.global_clouds, self.cloud_offset = local_clouds, local_clouds * self.world, 0
            return
        rank = dist.get_rank(self.group) if rank is None else rank
        counts = torch.zeros(self.world, dtype=torch.int64)
        counts[rank] = local_clouds
        if dist.get_backend(self.group) == "nccl":
            dev_counts = counts.cuda()
            dist.all_reduce(dev_counts, op=dist.ReduceOp.SUM, group=self.group)
            counts = dev_counts.cpu()
        else:
            dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=self.group)
        self.local_clouds, self.global_clouds = local_clouds, int(counts.sum())
        self.cloud_offset = int(counts[:rank].sum())

    def global_rows(self, rows: int) -> int:
        """Rows of the GLOBAL batch for a tensor that has `rows` rows on this rank (every such tensor has the same number
        of rows per cloud on every rank)."""
        assert rows % self.local_clouds == 0, (rows, self.local_clouds)
        return rows // self.local_clouds * self.global_clouds

    def allreduce(self, t: torch.Tensor) -> None:
        import torch.distributed as dist
        if self.staged:
            h = t.cpu()
            dist.all_reduce(h, op=dist.ReduceOp.SUM, group=self.group)
            t.copy_(h)
        else:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)


def _stats_totals(stats: torch.Tensor, nslots: int, C: int) -> torch.Tensor:
    out = torch.empty((1, 2, C), dtype=torch.float64, device=stats.device)
    H.check(H.lib().rl_bn_reduce_slots(stats.data_ptr(), nslots, C, out.data_ptr(), _st()), "rl_bn_reduce_slots")
    return out


def bn_finalize(stats, rows: int, tile: int, C: int, gamma, beta, rmean, rvar, nbt, momentum: float,
                eps: float, training: bool, sync: Optional[SyncGroup] = None, nslots: Optional[int] = None,
                folded_bias: Optional[torch.Tensor] = None, defer: Optional[list] = None, pivoted: bool = False,
                pivot: Optional[torch.Tensor] = None):
    """folded_bias: the layer's conv bias when the producing GEMM did NOT add it (rl_bn_finalize in rl_randlanet.h).
    pivoted: the partial sums are shifted around (m - folded_bias), m = `pivot` when given, else the running mean - the vector
    the producer was given, see gemm(pivot=...).
    pivot (training): the layer's pivot vector (Engine.Pv); the fold leaves this batch's mean of y there for the next step.
    defer (a list): the fold is only queued - the returned tensors are filled by `bn_finalize_flush(defer)`, which runs all
    queued folds as ONE launch; the caller flushes before anything reads them."""
    dev = gamma.device
    nslots = H.row_blocks(rows, tile) if nslots is None else nslots
    if training and sync is not None:            # batch statistics of the GLOBAL batch
        stats = _stats_totals(stats, nslots, C)
        if pivoted:
            # the ranks' sums are shifted around EACH RANK's pivot (its running mean - nothing forces the replicas' buffers to
            # be bit-equal): bring them to pivot 0 in double before they are added - S0 = S + n c, Q0 = Q + 2 c S + n c^2 with
            # the fp32 pivot c = running_mean - folded_bias the producer subtracted (exact in double up to 2^-53: the variance
            # keeps what the shift bought) - and finalize the totals as plain sums
            m = pivot if pivot is not None else rmean
            c = (m - folded_bias if folded_bias is not None else m).to(torch.float64)
            S, Q = stats[0, 0].clone(), stats[0, 1].clone()
            stats[0, 0] = S + rows * c
            stats[0, 1] = Q + 2.0 * c * S + rows * c * c
            pivoted = False
        sync.allreduce(stats)
        nslots, rows = 1, sync.global_rows(rows)
    scale = torch.empty(C, dtype=F32, device=dev)
    shift = torch.empty(C, dtype=F32, device=dev)
    mean = torch.empty(C, dtype=F32, device=dev) if training else None
    invstd = torch.empty(C, dtype=F32, device=dev) if training else None
    _dev_check(stats, gamma, beta, rmean, rvar, nbt, folded_bias, pivot)
    if not training:
        pivot = None
    assert folded_bias is None or folded_bias.numel() == C
    if defer is not None:
        it = H.BnFinalizeItem()
        it.stats, it.count, it.gamma, it.beta = H.ptr(stats), rows, H.ptr(gamma), H.ptr(beta)
        it.running_mean, it.running_var, it.num_batches_tracked = H.ptr(rmean), H.ptr(rvar), H.ptr(nbt)
        it.scale, it.shift, it.save_mean, it.save_invstd = scale.data_ptr(), shift.data_ptr(), H.ptr(mean), H.ptr(invstd)
        it.folded_bias, it.nslots, it.C, it.training, it.momentum, it.eps = H.ptr(folded_bias), nslots, C, int(training), momentum, eps
        it.pivoted = int(bool(pivoted and training))
        it.pivot = H.ptr(pivot)
        defer.append((it, stats, scale, shift, mean, invstd))       # (the tensors stay referenced until the launch is issued)
        return scale, shift, mean, invstd
    H.check(H.lib().rl_bn_finalize(H.ptr(stats), nslots, rows, C, H.ptr(gamma), H.ptr(beta),
                                   H.ptr(rmean), H.ptr(rvar), H.ptr(nbt), momentum, eps, int(training),
                                   scale.data_ptr(), shift.data_ptr(), H.ptr(mean), H.ptr(invstd), H.ptr(folded_bias),
                                   int(bool(pivoted and training)), H.ptr(pivot), _st()),
            "rl_bn_finalize")
    return scale, shift, mean, invstd


def bn_finalize_flush(defer: Optional[list]) -> None:
    """The queued BatchNorm folds as one launch (rl_bn_finalize_batch)."""
    if not defer:
        return
    arr = (H.BnFinalizeItem * len(defer))(*[d[0] for d in defer])
    H.check(H.lib().rl_bn_finalize_batch(arr, len(defer), _st()), "rl_bn_finalize_batch")
    defer.clear()


def _bn_bwd_desc(G: torch.Tensor, g_bstride: int, y: Lazy) -> H.BnBwdDesc:
    _dev_check(G, y.raw)
    assert G.dim() == 2 and G.shape[1] == y.raw.shape[1] and g_bstride == y.bstride, \
        "gradient must share the layout of the tensor it belongs to"
    assert G.shape[0] >= (y.B - 1) * y.bstride + y.n
    d = H.BnBwdDesc()
    d.G, d.Y, d.ld, d.bstride = G.data_ptr(), y.raw.data_ptr(), y.raw.shape[1], y.bstride
    d.B, d.n, d.C, d.act, d.slope = y.B, y.n, y.C, y.act, y.slope
    d.scale, d.shift, d.mean, d.invstd = H.ptr(y.scale), H.ptr(y.shift), H.ptr(y.mean), H.ptr(y.invstd)
    return d


def _bn_bwd_finalize(stats, slots: int, rows: int, Cc: int, dgamma, dbeta, coef, sync: Optional[SyncGroup],
                     also: Optional[list] = None) -> None:
    """dgamma / dbeta = this rank's sums; coef = the means the apply pass subtracts - of the GLOBAL batch with `sync`.
    also: queued finalizes of OTHER layers, tuples (stats, slots, rows, C, dgamma, dbeta, coef) whose sums are complete - they
    go out in this launch (rl_bn_bwd_finalize_batch) and the list is cleared."""
    if also and sync is None:
        todo = [(stats, slots, rows, Cc, dgamma, dbeta, coef)] + list(also)
        arr = (H.BnBwdFinalizeItem * len(todo))()
        for it, (s_, n_, r_, c_, dg_, db_, co_) in zip(arr, todo):
            it.stats, it.count, it.dgamma, it.dbeta, it.coef, it.nslots, it.C = s_.data_ptr(), r_, H.ptr(dg_), H.ptr(db_), co_.data_ptr(), n_, c_
        H.check(H.lib().rl_bn_bwd_finalize_batch(arr, len(todo), _st()), "rl_bn_bwd_finalize_batch")
        also.clear()
        return
    if also:
        for (s_, n_, r_, c_, dg_, db_, co_) in also:
            _bn_bwd_finalize(s_, n_, r_, c_, dg_, db_, co_, sync)
        also.clear()
    H.check(H.lib().rl_bn_bwd_finalize(stats.data_ptr(), slots, rows, Cc, H.ptr(dgamma), H.ptr(dbeta), coef.data_ptr(), _st()),
            "rl_bn_bwd_finalize")
    if sync is not None:
        tot = _stats_totals(stats, slots, Cc)
        sync.allreduce(tot)
        H.check(H.lib().rl_bn_bwd_finalize(tot.data_ptr(), 1, sync.global_rows(rows), Cc, None, None, coef.data_ptr(), _st()),
                "rl_bn_bwd_finalize")


def bn_backward(G: torch.Tensor, y: Lazy, dgamma: Optional[torch.Tensor], dbeta: Optional[torch.Tensor],
                training: bool, sync: Optional[SyncGroup] = None, stats: Optional[tuple] = None, also: Optional[list] = None) -> bool:
    """In place: G (gradient w.r.t. the activated value of `y`) becomes the gradient w.r.t. y.raw.
    stats: (partials, nslots) already left by the kernel that produced G (head_bwd) - no reduce sweep over G and Y here.
    also: other layers' queued backward finalizes (see _bn_bwd_finalize) to send out with this layer's; returns True when they
    went out (the list is then empty) - on the paths without a finalize launch of their own they stay queued."""
    d = _bn_bwd_desc(G, y.bstride, y)
    if stats is not None:
        assert training and y.mean is not None and sync is None
        coef = torch.empty(2 * y.C, dtype=F32, device=G.device)
        _bn_bwd_finalize(stats[0], stats[1], y.rows, y.C, dgamma, dbeta, coef, None, also=also)
        d.coef = coef.data_ptr()
        with _rec("bn_bwd_apply", (y.rows, y.C), 12 * y.rows * y.C, 0):
            H.check(H.lib().rl_bn_bwd_apply(C.byref(d), _st()), "rl_bn_bwd_apply")
        return not also
    if (training and y.mean is not None and sync is None and not NO_BN_SMALL and G.data_ptr() % 16 == 0 and y.raw.data_ptr() % 16 == 0
            and H.lib().rl_bn_bwd_fused_supported(y.rows, y.C, y.raw.shape[1])):
        # a small tensor: reduce, finalize and apply in one launch (a workgroup owns a channel quad and all its rows)
        with _rec("bn_bwd_fused", (y.rows, y.C), 12 * y.rows * y.C, 0):
            H.check(H.lib().rl_bn_bwd_fused(C.byref(d), y.rows, H.ptr(dgamma), H.ptr(dbeta), None, _st()), "rl_bn_bwd_fused")
        return not also
    if training and y.mean is not None:
        stats = new_stats(G.device, y.C)
        coef = torch.empty(2 * y.C, dtype=F32, device=G.device)
        d.stats = stats.data_ptr()
        with _rec("bn_bwd_reduce", (y.rows, y.C), 8 * y.rows * y.C, 0):
            H.check(H.lib().rl_bn_bwd_reduce(C.byref(d), _st()), "rl_bn_bwd_reduce")
        _bn_bwd_finalize(stats, H.lib().rl_bn_bwd_slots(y.rows), y.rows, y.C, dgamma, dbeta, coef, sync, also=also)
        d.coef = coef.data_ptr()
    with _rec("bn_bwd_apply", (y.rows, y.C), 12 * y.rows * y.C, 0):
        H.check(H.lib().rl_bn_bwd_apply(C.byref(d), _st()), "rl_bn_bwd_apply")
    return not also


def resid_bn_supported(y1: Lazy, y2: Lazy) -> bool:
    dense = all(y.bstride == y.n and y.raw.shape == (y.B * y.n, y.C) and y.mean is not None and y.act == H.ACT_NONE for y in (y1, y2))
    return dense and y1.C == y2.C and y1.rows == y2.rows and bool(H.lib().rl_resid_bn_bwd_supported(y1.rows, y1.C))


def resid_bn_backward(G: torch.Tensor, O: torch.Tensor, slope: float, y1: Lazy, y2: Lazy, dgamma1, dbeta1, dgamma2, dbeta2,
                      sync: Optional[SyncGroup] = None):
    """Backward of O = LeakyReLU(BN1(y1) + BN2(y2)) down to the two raw tensors: G (dL/dO) becomes the gradient
    w.r.t. y1.raw in place, the returned tensor is the gradient w.r.t. y2.raw (modules.py:325 + two BatchNorm2d)."""
    _dev_check(G, O, y1.raw, y2.raw)
    rows, Cc = y1.rows, y1.C
    assert G.shape == O.shape == (rows, Cc)
    d = H.ResidBnBwdDesc()
    G2 = torch.empty_like(G)
    d.G, d.G2, d.O, d.slope, d.rows, d.C = G.data_ptr(), G2.data_ptr(), O.data_ptr(), slope, rows, Cc
    d.Y1, d.scale1, d.mean1, d.invstd1 = y1.raw.data_ptr(), y1.scale.data_ptr(), y1.mean.data_ptr(), y1.invstd.data_ptr()
    d.Y2, d.scale2, d.mean2, d.invstd2 = y2.raw.data_ptr(), y2.scale.data_ptr(), y2.mean.data_ptr(), y2.invstd.data_ptr()
    if sync is None and not NO_BN_SMALL and H.lib().rl_resid_bn_bwd_fused_supported(rows, Cc):
        with _rec("resid_bn_bwd_fused", (rows, Cc), 24 * rows * Cc, 0):
            H.check(H.lib().rl_resid_bn_bwd_fused(C.byref(d), H.ptr(dgamma1), H.ptr(dbeta1), H.ptr(dgamma2), H.ptr(dbeta2), _st()),
                    "rl_resid_bn_bwd_fused")
        return G2
    st1, st2 = new_stats(G.device, Cc), new_stats(G.device, Cc)
    c1 = torch.empty(2 * Cc, dtype=F32, device=G.device)
    c2 = torch.empty(2 * Cc, dtype=F32, device=G.device)
    d.stats1, d.stats2, d.coef1, d.coef2 = st1.data_ptr(), st2.data_ptr(), c1.data_ptr(), c2.data_ptr()
    with _rec("resid_bn_bwd_reduce", (rows, Cc), 16 * rows * Cc, 0):
        H.check(H.lib().rl_resid_bn_bwd_reduce(C.byref(d), _st()), "rl_resid_bn_bwd_reduce")
    slots = H.lib().rl_bn_bwd_slots(rows)
    if sync is None:
        H.check(H.lib().rl_bn_bwd_finalize_pair(st1.data_ptr(), st2.data_ptr(), slots, rows, Cc, H.ptr(dgamma1), H.ptr(dbeta1), c1.data_ptr(),
                                                H.ptr(dgamma2), H.ptr(dbeta2), c2.data_ptr(), _st()), "rl_bn_bwd_finalize_pair")
    else:
        _bn_bwd_finalize(st1, slots, rows, Cc, dgamma1, dbeta1, c1, sync)
        _bn_bwd_finalize(st2, slots, rows, Cc, dgamma2, dbeta2, c2, sync)
    with _rec("resid_bn_bwd_apply", (rows, Cc), 24 * rows * Cc, 0):
        H.check(H.lib().rl_resid_bn_bwd_apply(C.byref(d), _st()), "rl_resid_bn_bwd_apply")
    return G2


# ------------------------------------------------------------------------------------ rows
def _rows_desc(src: torch.Tensor, src_cols: Tuple[int, int], src_bstride: int, dst: torch.Tensor,
               dst_cols: Tuple[int, int], rows: int, rows_per_batch: int, *, index=None,
               index_shared: bool = False, accumulate: bool = False, lazy: Optional[Lazy] = None):
    _dev_check(src, dst, index)
    d = H.RowsDesc()
    es = src.element_size()
    assert src.dtype == F32 and dst.dtype == F32 and src.dim() == 2 and dst.dim() == 2
    c0s, cn = src_cols
    c0d, cn2 = dst_cols
    assert cn == cn2 and c0s + cn <= src.shape[1] and c0d + cn <= dst.shape[1] and dst.shape[0] >= rows
    d.src, d.lds, d.src_bstride = src.data_ptr() + c0s * es, src.shape[1], src_bstride
    d.dst, d.ldd = dst.data_ptr() + c0d * es, dst.shape[1]
    d.rows, d.rows_per_batch, d.C = rows, rows_per_batch, cn
    if index is not None:
        if index.dtype == torch.int32:
            d.index32 = index.data_ptr()
        else:
            assert index.dtype == torch.int64
            d.index64 = index.data_ptr()
        assert index.numel() >= (rows_per_batch if index_shared else rows)
    d.index_shared, d.accumulate = int(index_shared), int(accumulate)
    if lazy is not None and lazy.scale is not None:
        assert c0s == 0 and cn == lazy.C
        d.scale, d.shift, d.act, d.slope = lazy.scale.data_ptr(), lazy.shift.data_ptr(), lazy.act, lazy.slope
    return d, (8 + 4 * int(accumulate)) * rows * cn


def copy_rows(src: torch.Tensor, src_cols: Tuple[int, int], src_bstride: int, dst: torch.Tensor,
              dst_cols: Tuple[int, int], rows: int, rows_per_batch: int, *, index=None,
              index_shared: bool = False, accumulate: bool = False, lazy: Optional[Lazy] = None) -> None:
    """dst[r, dst_cols] (=|+=) f(src[b*src_bstride + idx, src_cols]); column ranges are (start, count)."""
    d, nbytes = _rows_desc(src, src_cols, src_bstride, dst, dst_cols, rows, rows_per_batch, index=index,
                           index_shared=index_shared, accumulate=accumulate, lazy=lazy)
    with _rec("copy_rows", (rows, src_cols[1], index is not None), nbytes, 0):
        H.check(H.lib().rl_copy_rows(C.byref(d), _st()), "rl_copy_rows")


def copy_rows_pair(a: tuple, b: tuple) -> None:
    """Two independent copy_rows in one launch: a, b = (args, kwargs) of copy_rows (the two halves of a concat)."""
    d0, n0 = _rows_desc(*a[0], **a[1])
    d1, n1 = _rows_desc(*b[0], **b[1])
    with _rec("copy_rows_pair", (a[0][5], a[0][1][1], b[0][1][1]), n0 + n1, 0):
        H.check(H.lib().rl_copy_rows_pair(C.byref(d0), C.byref(d1), _st()), "rl_copy_rows_pair")


def scatter_add_rows(src: torch.Tensor, src_cols: Tuple[int, int], dst: torch.Tensor, dst_bstride: int,
                     rows: int, rows_per_batch: int, index: torch.Tensor, index_shared: bool = False) -> None:
    """dst[b*dst_bstride + index[r], :] += src[r, src_cols] (fp32 atomics; dst zeroed by the caller)."""
    _dev_check(src, dst, index)
    d = H.RowsDesc()
    c0s, cn = src_cols
    assert cn == dst.shape[1] and c0s + cn <= src.shape[1] and src.shape[0] >= rows
    d.src, d.lds, d.src_bstride = src.data_ptr() + c0s * 4, src.shape[1], dst_bstride
    d.dst, d.ldd = dst.data_ptr(), dst.shape[1]
    d.rows, d.rows_per_batch, d.C = rows, rows_per_batch, cn
    if index.dtype == torch.int32:
        d.index32 = index.data_ptr()
    else:
        d.index64 = index.data_ptr()
    d.index_shared = int(index_shared)
    with _rec("scatter_add", (rows, cn), 12 * rows * cn, 0):
        H.check(H.lib().rl_scatter_add_rows(C.byref(d), _st()), "rl_scatter_add_rows")


@dataclass
class Csr:
    """Transpose of a neighbour graph idx (B, n_src, k) -> for destination (b, j) the local source rows i*k + kk that
    gathered it, ascending (rl_csr_build)."""
    offsets: torch.Tensor   # (B, n_dst + 1) int32
    entries: torch.Tensor   # (B, n_src*k) int32
    B: int
    n_src: int
    k: int
    n_dst: int


def csr_build(graphs):
    """graphs: list of (idx int32 (B, n_src, k), n_dst).  One launch set for all of them."""
    out = []
    for c0 in range(0, len(graphs), H.CSR_MAX_TASKS):
        chunk = graphs[c0:c0 + H.CSR_MAX_TASKS]
        arr = (H.CsrTask * len(chunk))()
        res = []
        B = chunk[0][0].shape[0]
        nent = 0
        for t, (idx, n_dst) in zip(arr, chunk):
            _dev_check(idx)
            assert idx.dtype == torch.int32 and idx.dim() == 3 and idx.shape[0] == B and n_dst > 0
            _, n_src, k = idx.shape
            off = torch.empty((B, n_dst + 1), dtype=torch.int32, device=idx.device)
            ent = torch.empty((B, n_src * k), dtype=torch.int32, device=idx.device)
            t.idx, t.n_src, t.k, t.n_dst, t.offsets, t.entries = idx.data_ptr(), n_src, k, n_dst, off.data_ptr(), ent.data_ptr()
            res.append(Csr(off, ent, B, n_src, k, n_dst))
            nent += B * n_src * k
        nbytes = H.lib().rl_csr_workspace_bytes(arr, len(chunk), B)
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=chunk[0][0].device)
        with _rec("csr_build", (len(chunk), nent), 16 * nent, 0):
            H.check(H.lib().rl_csr_build(arr, len(chunk), B, ws.data_ptr(), ws.numel(), _st()), "rl_csr_build")
        out.extend(res)
    return out


def segment_sum_rows(src: torch.Tensor, src_cols: Tuple[int, int], src_bstride: int, csr: Csr, dst: torch.Tensor,
                     dst_bstride: int, accumulate: bool = False) -> None:
    """dst[b*dst_bstride + j, :] (=|+=) sum of src[b*src_bstride + r, src_cols] over the rows r that gathered (b, j), in
    ascending r - the gather's backward in a fixed order (no atomics, first writer needs no zero fill)."""
    _dev_check(src, dst, csr.offsets, csr.entries)
    c0, cn = src_cols
    assert src.dtype in (F32, BF16) and dst.dtype == F32 and src.dim() == 2 and dst.dim() == 2
    assert c0 + cn <= src.shape[1] and cn == dst.shape[1]
    assert src.shape[0] >= (csr.B - 1) * src_bstride + csr.n_src * csr.k
    assert dst.shape[0] >= (csr.B - 1) * dst_bstride + csr.n_dst
    d = H.SegsumDesc()
    d.src, d.lds, d.src_bstride = src.data_ptr() + src.element_size() * c0, src.shape[1], src_bstride
    d.src_bf16 = int(src.dtype == BF16)
    d.dst, d.ldd, d.dst_bstride = dst.data_ptr(), dst.shape[1], dst_bstride
    d.offsets, d.entries, d.entries_per_cloud = csr.offsets.data_ptr(), csr.entries.data_ptr(), csr.n_src * csr.k
    d.B, d.n_dst, d.C, d.accumulate = csr.B, csr.n_dst, cn, int(accumulate)
    rows = csr.B * csr.n_src * csr.k
    with _rec("segment_sum", (rows, cn), cn * (src.element_size() * rows + 4 * csr.B * csr.n_dst * (2 if accumulate else 1)) + 4 * rows, 0):
        H.check(H.lib().rl_segment_sum_rows(C.byref(d), _st()), "rl_segment_sum_rows")


# ------------------------------------------------------------------------- pooling, residual
@dataclass
class VirtualRpe:
    """The rpe branch of one encoder level as a function of the coordinates (never stored): stage 1 =
    relu(bn1(rpe . W1^T + b1)), stage 2 = relu(bn2(stage1 . W2^T + b2)) (reference modules.py:313-320).  bn1 / bn2 are
    filled in by the engine once their batch statistics are known: Lazy-like records (scale, shift, mean, invstd)."""
    xyz: torch.Tensor
    idx: torch.Tensor
    d2: torch.Tensor
    B: int
    n: int
    h: int
    W1: torch.Tensor
    b1: torch.Tensor
    W2: torch.Tensor
    b2: torch.Tensor
    bn1: Optional[Lazy] = None
    bn2: Optional[Lazy] = None
    # training: the running means of the two BatchNorms - pivots of the shifted batch statistics (rl_pool_desc.pivot_mean*)
    piv1: Optional[torch.Tensor] = None
    piv2: Optional[torch.Tensor] = None

    @property
    def rows(self) -> int:
        return self.B * self.n * 16


def virtual_rpe_supported(d: int, K: int, points: int = 0, n: int = 0) -> bool:
    """points / n (when given): the kernels of a virtual branch address through 32-bit byte offsets - (points*16) x d/2 row
    tensors below 2 GB, clouds below 2^24 points; larger levels take the stored path."""
    if points * 16 * (d // 2) * 4 >= 2 ** 31 or n >= 2 ** 24:
        return False
    return K == 16 and d in (16, 32, 64) and pool_supported(d, K)


def _fill_virtual(pd: "H.PoolDesc", v: VirtualRpe, stage: int) -> None:
    _dev_check(v.xyz, v.idx, v.d2, v.W1, v.b1, v.W2, v.b2)
    assert v.idx.dtype == torch.int32 and v.idx.shape == (v.B, v.n, 16) and v.d2.shape == v.idx.shape
    assert v.xyz.shape[0] == v.B and v.xyz.shape[1] >= v.n and v.xyz.shape[2] in (3, 4)
    pd.xyz_width = v.xyz.shape[2]
    assert v.W1.numel() == v.h * 10 and v.b1.numel() == v.h and v.W2.numel() == v.h * v.h and v.b2.numel() == v.h
    pd.u_source, pd.xyz, pd.xyz_bstride, pd.nbr_d2 = stage, v.xyz.data_ptr(), v.xyz.shape[1], v.d2.data_ptr()
    pd.W1, pd.b1, pd.W2, pd.b2 = v.W1.data_ptr(), v.b1.data_ptr(), v.W2.data_ptr(), v.b2.data_ptr()
    pd.idx, pd.points, pd.n, pd.d, pd.nbr_k = v.idx.data_ptr(), v.B * v.n, v.n, 2 * v.h, 16
    _dev_check(v.piv1, v.piv2)
    pd.pivot_mean1, pd.pivot_mean2 = H.ptr(v.piv1), H.ptr(v.piv2)
    for tag, bn in (("1", v.bn1), ("2", v.bn2)):
        if bn is not None:
            _dev_check(bn.scale, bn.shift, bn.mean, bn.invstd)
            setattr(pd, f"scale{tag}", bn.scale.data_ptr())
            setattr(pd, f"shift{tag}", bn.shift.data_ptr())
            setattr(pd, f"mean{tag}", H.ptr(bn.mean))
            setattr(pd, f"invstd{tag}", H.ptr(bn.invstd))


def rpe_stats(v: VirtualRpe, stage: int):
    """BatchNorm partial statistics of the raw output of stage 1 / 2 of the virtual rpe branch: (stats, nslots)."""
    pd = H.PoolDesc()
    _fill_virtual(pd, v, stage)
    assert stage == 1 or v.bn1 is not None
    nslots = H.lib().rl_rpe_stats_slots(v.B * v.n)
    stats = torch.empty((nslots, 2, v.h), dtype=torch.float64, device=v.xyz.device)
    with _rec("rpe_stats", (v.rows, v.h, stage), 8 * v.rows, 2 * v.rows * (16 * v.h + (v.h * v.h if stage == 2 else 0))):
        H.check(H.lib().rl_rpe_stats(C.byref(pd), stats.data_ptr(), _st()), "rl_rpe_stats")
    return stats, nslots


def rpe_bn_backward(v: VirtualRpe, stage: int, G: torch.Tensor, dgamma, dbeta, sync: Optional[SyncGroup] = None,
                    stats: Optional[torch.Tensor] = None, nslots: int = 0, queue: Optional[list] = None) -> torch.Tensor:
    """BatchNorm backward statistics of virtual stage `stage` from G (gradient w.r.t. its activated output): fills
    dgamma / dbeta and returns coef (2h floats) for rpe_wgrad.  `stats` / `nslots`: partials already produced by the
    pooling backward kernel that completed G (pool_bwd's bn_bwd_stats) - then no pass over G is made here."""
    if stats is None:
        pd = H.PoolDesc()
        _fill_virtual(pd, v, stage)
        _dev_check(G)
        assert G.shape == (v.rows, v.h) and G.dtype in (F32, BF16)
        pd.rows_bf16 = int(G.dtype == BF16)
        nslots = H.lib().rl_rpe_stats_slots(v.B * v.n)
        stats = torch.empty((nslots, 2, v.h), dtype=torch.float64, device=G.device)
        with _rec("rpe_bn_reduce", (v.rows, v.h, stage), 4 * v.rows * v.h + 8 * v.rows, 0):
            H.check(H.lib().rl_rpe_bn_reduce(C.byref(pd), G.data_ptr(), stats.data_ptr(), _st()), "rl_rpe_bn_reduce")
    coef = torch.empty(2 * v.h, dtype=F32, device=G.device)
    if queue is not None and sync is None:
        queue.append((stats, nslots, v.rows, v.h, dgamma, dbeta, coef))       # goes out with the next layer's finalize launch
    else:
        _bn_bwd_finalize(stats, nslots, v.rows, v.h, dgamma, dbeta, coef, sync)
    return coef


def rpe_wgrad(v: VirtualRpe, stage: int, G: torch.Tensor, coef: torch.Tensor, dW: torch.Tensor, dbias: torch.Tensor,
              pending: list, GU1: Optional[torch.Tensor] = None) -> None:
    """Weight / bias gradient of the stage's Linear (queued on `pending` for the batched slab reduction) and, for stage 2,
    GU1 = the gradient w.r.t. the activated stage-1 output."""
    pd = H.PoolDesc()
    _fill_virtual(pd, v, stage)
    _dev_check(G, coef, dW, dbias, GU1)
    Kin = 10 if stage == 1 else v.h
    assert dW.numel() == v.h * Kin and dbias.numel() == v.h and (stage == 1 or GU1.shape == (v.rows, v.h))
    assert G.dtype in (F32, BF16) and (GU1 is None or GU1.dtype == G.dtype)
    pd.rows_bf16 = int(G.dtype == BF16)
    es = G.element_size()
    floats = H.lib().rl_rpe_wgrad_slab_floats(v.B * v.n, 2 * v.h, stage)
    slab = torch.empty(floats, dtype=F32, device=G.device)
    with _rec("rpe_wgrad", (v.rows, Kin, v.h), es * v.rows * v.h * (2 if stage == 2 else 1) + 8 * v.rows, 2 * v.rows * v.h * (Kin + (v.h if stage == 2 else 0))):
        H.check(H.lib().rl_rpe_wgrad(C.byref(pd), G.data_ptr(), coef.data_ptr(), slab.data_ptr(), slab.numel(), H.ptr(GU1), _st()),
                "rl_rpe_wgrad")
    it = H.WgradReduceItem()
    it.slab, it.dW, it.dbias, it.w_ks, it.w_ns = slab.data_ptr(), dW.data_ptr(), dbias.data_ptr(), 1, Kin
    it.nsplit, it.N, it.K = H.lib().rl_rpe_stats_slots(v.B * v.n), v.h, Kin
    pending.append((it, slab, dW, dbias))


def pool_supported(d: int, K: int) -> bool:
    return bool(H.lib().rl_pool_supported(d, K))


def _pool_desc(u, g: Lazy, idx: torch.Tensor, W: torch.Tensor, n: int, d: int, stage: int = 0) -> H.PoolDesc:
    """u: the rpe-branch half of X - a Lazy tensor ((points*16) x d/2), or a VirtualRpe with `stage` 1 / 2."""
    _dev_check(g.raw, idx, W, g.scale, g.shift)
    h = d // 2
    B = u.B
    assert idx.dtype == torch.int32 and idx.shape == (B, n, 16)
    assert g.raw.shape[1] == h and g.C == h and g.n == n and g.raw.shape[0] >= (B - 1) * g.bstride + n
    assert W.numel() == d * d
    pd = H.PoolDesc()
    if isinstance(u, VirtualRpe):
        assert stage in (1, 2) and u.h == h and u.n == n and u.bn1 is not None and (stage == 1 or u.bn2 is not None)
        _fill_virtual(pd, u, stage)
    else:
        _dev_check(u.raw, u.scale, u.shift)
        assert u.raw.shape == (B * n * 16, h) and u.bstride == u.n == n * 16 and u.C == h
        pd.U, pd.u_scale, pd.u_shift, pd.u_act, pd.u_slope = u.raw.data_ptr(), H.ptr(u.scale), H.ptr(u.shift), u.act, u.slope
    pd.G, pd.g_bstride = g.raw.data_ptr(), g.bstride
    pd.g_scale, pd.g_shift, pd.g_act, pd.g_slope = H.ptr(g.scale), H.ptr(g.shift), g.act, g.slope
    pd.idx, pd.W, pd.points, pd.n, pd.d, pd.nbr_k = idx.data_ptr(), W.data_ptr(), B * n, n, d, 16
    return pd


def pool_fwd(u, g: Lazy, idx: torch.Tensor, W: torch.Tensor, n: int, d: int, stage: int = 0, next_stats: bool = False):
    """Fused gather+concat -> score Linear -> softmax over K -> weighted sum: (B*n, d).  next_stats (virtual stage 1 only):
    also returns the BatchNorm partial statistics of the raw stage-2 output as (pooled, stats, nslots)."""
    pd = _pool_desc(u, g, idx, W, n, d, stage)
    stats2 = None
    if next_stats:
        assert stage == 1
        ns = H.lib().rl_pool_fwd_slots(u.B * n, d)
        stats2 = torch.empty((ns, 2, d // 2), dtype=torch.float64, device=W.device)
        pd.bn_fwd_stats2 = stats2.data_ptr()
    out = torch.empty((u.B * n, d), dtype=F32, device=W.device)
    pd.Pout = out.data_ptr()
    P = u.B * n
    virt = isinstance(u, VirtualRpe)
    # (virtual: index, distance, output + gathered coordinates and rows - DESIGN.md section 5)
    fbytes = P * (4 * (32 + d) + 16 * (16 + 4 * (d // 2))) if virt else 4 * (2 * P * 16 * (d // 2) + P * 16 + P * d)
    with _rec("pool_fwd_virtual" if virt else "pool_fwd", (P, 16, d), fbytes, 2 * P * 16 * d * d):
        H.check(H.lib().rl_pool_fwd(C.byref(pd), _st()), "rl_pool_fwd")
    if next_stats:
        return out, stats2, ns
    return out


def pool_bwd(u, g: Lazy, idx: torch.Tensor, W: torch.Tensor, n: int, d: int, dP: torch.Tensor,
             GU: torch.Tensor, gu_accumulate: bool, dW: torch.Tensor, pending: Optional[list] = None,
             stage: int = 0, bn_bwd_stats: Optional[torch.Tensor] = None, batch: Optional[list] = None) -> torch.Tensor:
    """Backward of the fused pooling block.  Returns DG ((points*16) x d/2): the gradient of the gathered row of every
    neighbourhood slot, to be summed per gathered point with segment_sum_rows.  d <= 64: dW comes out of the kernel.
    d = 128: the kernel writes dS and the weight gradient is the ordinary wide kernel (queued on `pending` like every other
    layer's) on X - which it reads in place from u, g and idx (ConcatGather) where rl_wgrad supports that and get_pool128_x()
    says so, and from a copy the pooling kernel stores otherwise."""
    pd = _pool_desc(u, g, idx, W, n, d, stage)
    _dev_check(dP, GU, dW)
    P = u.B * n
    assert dP.shape == (P, d) and GU.shape == (P * 16, d // 2) and dW.numel() == d * d
    rdt = row_dtype()
    virt = isinstance(u, VirtualRpe)
    assert GU.dtype == (rdt if virt else F32), "GU: the row storage type under a virtual rpe branch, fp32 for a real U tensor"
    pd.rows_bf16 = int(rdt == BF16)
    es = 2 if rdt == BF16 else 4
    DG = torch.empty((P * 16, d // 2), dtype=rdt, device=W.device)
    if bn_bwd_stats is not None:
        _dev_check(bn_bwd_stats)
        assert stage > 0 and bn_bwd_stats.dtype == torch.float64
        assert bn_bwd_stats.numel() >= H.lib().rl_pool_bwd_slots(P, d) * d
        pd.bn_bwd_stats = bn_bwd_stats.data_ptr()
    pd.dP, pd.GU, pd.gu_accumulate, pd.DG, pd.dW = dP.data_ptr(), GU.data_ptr(), int(gu_accumulate), DG.data_ptr(), dW.data_ptr()
    # algorithmic bytes.  Virtual rpe half: per point the forward's 4*(32 + d) (index, distance, output) +
    # 16*(16 + 4*d/2) (gathered coordinates and rows), + 4*d (dP) + DG and GU rows (GU read first when accumulating).  A real U
    # tensor: its rows instead of the coordinates and distances.
    h = d // 2
    if virt:
        nbytes = P * (4 * (32 + d) + 16 * (16 + 4 * h) + 4 * d + es * 16 * h * (2 + int(gu_accumulate)))
    else:
        nbytes = (4 * (2 * P * 16 * h + P * 16 + 2 * P * d) + es * P * 16 * h + 4 * P * 16 * h * (1 + int(gu_accumulate)))
    if d == 128:
        dS = torch.empty((P * 16, d), dtype=rdt, device=W.device)
        xop = ConcatGather(u, g, idx) if (rdt == F32 and not virt and get_pool128_x() == "in_place") else None
        if xop is not None and not wgrad_supported(xop, dS, n * 16, d):
            xop = None
        if xop is None:
            X = torch.empty((P * 16, d), dtype=rdt, device=W.device)
            pd.X_out, xop = X.data_ptr(), plain(X, u.B, n * 16)
        else:
            pd.x_optional = 1
        pd.dS_out = dS.data_ptr()
        with _rec("pool_bwd", (P, 16, d), nbytes + (1 + int(pd.x_optional == 0)) * es * P * 16 * d, 4 * P * 16 * d * d):
            H.check(H.lib().rl_pool_bwd(C.byref(pd), _st()), "rl_pool_bwd")
        wgrad(xop, dS, n * 16, d, dW, 1, d, None, pending=pending, batch=batch)
        return DG
    floats = H.lib().rl_pool_slab_floats(P, d)
    if pending is not None:
        # the partial dW slabs join the backward pass's ONE slab reduction (wgrad_flush) instead of a launch of their own
        slab = torch.empty(floats, dtype=F32, device=W.device)
        pd.dW = None
    else:
        slab = _slab(W.device, floats)
    pd.slab, pd.slab_floats = slab.data_ptr(), slab.numel()
    with _rec("pool_bwd", (P, 16, d), nbytes, 6 * P * 16 * d * d):
        H.check(H.lib().rl_pool_bwd(C.byref(pd), _st()), "rl_pool_bwd")
    if pending is not None:
        it = H.WgradReduceItem()
        it.slab, it.dW, it.dbias, it.w_ks, it.w_ns = slab.data_ptr(), dW.data_ptr(), None, 1, d
        it.nsplit, it.N, it.K = H.lib().rl_pool_bwd_grid(P, d, int(virt)), d, d
        pending.append((it, slab, dW, None))
    return DG


def _attpool_src(x: ConcatGather) -> H.AttpoolSrc:
    u, g, idx = x.u, x.g, x.idx
    _dev_check(u.raw, u.scale, u.shift, g.raw, g.scale, g.shift, idx)
    assert idx.dtype == torch.int32 and idx.numel() == u.rows and u.bstride == u.n and g.B == u.B and u.C == g.C
    assert u.raw.dtype == F32 and g.raw.dtype == F32 and u.raw.shape[0] >= u.rows and u.raw.shape[1] >= u.C
    assert g.raw.shape[0] >= (g.B - 1) * g.bstride + g.n and g.raw.shape[1] >= g.C, "second source rows out of range"
    d = H.AttpoolSrc()
    d.U, d.ldu, d.G, d.ldg, d.g_bstride = u.raw.data_ptr(), u.raw.shape[1], g.raw.data_ptr(), g.raw.shape[1], g.bstride
    if u.scale is not None:
        d.u_scale, d.u_shift, d.u_act, d.u_slope = u.scale.data_ptr(), u.shift.data_ptr(), u.act, u.slope
    if g.scale is not None:
        d.g_scale, d.g_shift, d.g_act, d.g_slope = g.scale.data_ptr(), g.shift.data_ptr(), g.act, g.slope
    assert u.n % 16 == 0
    d.idx, d.n, d.h = idx.data_ptr(), u.n // 16, u.C
    return d


def attpool_concat_supported(x: ConcatGather, P: int, K: int) -> bool:
    """Do rl_attpool_fwd_cat / rl_attpool_bwd_cat take these sources (rl_attpool_cat_supported: nothing is launched)?  Only what
    the descriptor cannot say is answered here: fp32 rows in both sources, a contiguous U, halves of one width."""
    if not (x.u.raw.dtype == F32 and x.g.raw.dtype == F32 and x.u.bstride == x.u.n and x.u.C == x.g.C and x.u.n % 16 == 0):
        return False
    rc = H.lib().rl_attpool_cat_supported(C.byref(_attpool_src(x)), P, K, x.C)
    if rc not in (0, H.ERR_UNSUPPORTED):     # (a query, not a launch: only a malformed descriptor is reported)
        H.check(rc, "rl_attpool_cat_supported")
    return rc == 0


def attpool_fwd(X, S: torch.Tensor, P: int, K: int) -> torch.Tensor:
    """X: the stored (P*K, C) tensor, or a ConcatGather - its two halves read where they live (rl_attpool_fwd_cat)."""
    cat = isinstance(X, ConcatGather)
    Cc = X.C if cat else X.shape[1]
    assert S.shape == (P * K, Cc)
    out = torch.empty((P, Cc), dtype=F32, device=S.device)
    if cat:         # the U half, the gathered table once (it stays in L2), one index per row; S; Pout
        src = _attpool_src(X)
        _dev_check(S)
        with _rec("attpool_fwd", (P, K, Cc), 4 * (P * K * X.u.C + X.g.rows * X.g.C + P * K + P * K * Cc + P * Cc), 0):
            H.check(H.lib().rl_attpool_fwd_cat(C.byref(src), S.data_ptr(), P, K, Cc, out.data_ptr(), _st()), "rl_attpool_fwd_cat")
        return out
    _dev_check(X, S)
    assert X.shape == S.shape
    with _rec("attpool_fwd", (P, K, Cc), 4 * (2 * P * K * Cc + P * Cc), 0):
        H.check(H.lib().rl_attpool_fwd(X.data_ptr(), S.data_ptr(), P, K, Cc, out.data_ptr(), _st()), "rl_attpool_fwd")
    return out


def attpool_bwd(X, S, Pout, dP, P: int, K: int):
    cat = isinstance(X, ConcatGather)
    Cc = X.C if cat else X.shape[1]
    _dev_check(S, Pout, dP)
    assert S.shape == (P * K, Cc) and Pout.shape == dP.shape == (P, Cc)
    dS = torch.empty_like(S)
    dXa = torch.empty_like(S)
    if cat:
        src = _attpool_src(X)
        with _rec("attpool_bwd", (P, K, Cc), 4 * (P * K * X.u.C + X.g.rows * X.g.C + P * K + 3 * P * K * Cc + 2 * P * Cc), 0):
            H.check(H.lib().rl_attpool_bwd_cat(C.byref(src), S.data_ptr(), Pout.data_ptr(), dP.data_ptr(), P, K, Cc,
                                               dS.data_ptr(), dXa.data_ptr(), _st()), "rl_attpool_bwd_cat")
        return dS, dXa
    _dev_check(X)
    assert X.shape == S.shape and X.dtype == S.dtype
    with _rec("attpool_bwd", (P, K, Cc), 4 * (4 * P * K * Cc + 2 * P * Cc), 0):
        H.check(H.lib().rl_attpool_bwd(X.data_ptr(), S.data_ptr(), Pout.data_ptr(), dP.data_ptr(), P, K, Cc,
                                       dS.data_ptr(), dXa.data_ptr(), _st()), "rl_attpool_bwd")
    return dS, dXa


def add_act_fwd(y1: Lazy, y2: Lazy, slope: float) -> torch.Tensor:
    assert y1.rows == y2.rows and y1.C == y2.C and y1.bstride == y1.n and y2.bstride == y2.n
    out = torch.empty((y1.rows, y1.C), dtype=F32, device=y1.raw.device)
    with _rec("add_act", (y1.rows, y1.C), 12 * y1.rows * y1.C, 0):
        H.check(H.lib().rl_add_act_fwd(y1.raw.data_ptr(), y1.scale.data_ptr(), y1.shift.data_ptr(), y2.raw.data_ptr(),
                                       y2.scale.data_ptr(), y2.shift.data_ptr(), y1.rows, y1.C, slope, out.data_ptr(),
                                       _st()), "rl_add_act_fwd")
    return out


def add_act_bwd(G: torch.Tensor, O: torch.Tensor, slope: float) -> None:
    assert G.shape == O.shape and G.is_contiguous() and O.is_contiguous()
    with _rec("add_act", (G.shape[0], G.shape[1]), 12 * G.numel(), 0):
        H.check(H.lib().rl_add_act_bwd(G.data_ptr(), O.data_ptr(), G.shape[0], G.shape[1], slope, _st()), "rl_add_act_bwd")


def scale_mask(x: torch.Tensor, mask: torch.Tensor, scale: float) -> None:
    _dev_check(x, mask)
    assert mask.dtype == torch.uint8 and mask.numel() == x.numel() and x.dtype == F32
    H.check(H.lib().rl_scale_mask(x.data_ptr(), mask.data_ptr(), scale, x.numel(), _st()), "rl_scale_mask")


def dropout_tick(counter: torch.Tensor) -> torch.Tensor:
    """counter[0] += 1 on the device; returns a fresh device scalar holding the new value - the key of one pass's mask."""
    _dev_check(counter)
    assert counter.dtype == torch.int64 and counter.numel() == 1
    key = torch.empty(1, dtype=torch.int64, device=counter.device)
    H.check(H.lib().rl_dropout_tick(counter.data_ptr(), key.data_ptr(), _st()), "rl_dropout_tick")
    return key


def dropout_fwd(x: Lazy, key: torch.Tensor, seed: int, p: float, first_row: int = 0) -> torch.Tensor:
    """Dropout of the (activated) dense tensor x with the Philox mask of (seed, key): (rows, C) output.  first_row: where
    this tensor's row 0 sits in the whole batch's tensor (shards of one batch draw slices of one mask)."""
    _dev_check(x.raw, x.scale, x.shift, key)
    assert x.bstride == x.n and x.raw.shape == (x.rows, x.C) and x.C % 4 == 0
    out = torch.empty_like(x.raw)
    with _rec("dropout", (x.rows, x.C), 8 * x.rows * x.C, 0):
        H.check(H.lib().rl_dropout_fwd(x.raw.data_ptr(), H.ptr(x.scale), H.ptr(x.shift), x.act, x.slope, out.data_ptr(),
                                       x.rows, first_row, x.C, key.data_ptr(), seed & 0xFFFFFFFFFFFFFFFF, p, _st()), "rl_dropout_fwd")
    return out


def dropout_bwd(G: torch.Tensor, key: torch.Tensor, seed: int, p: float, first_row: int = 0) -> None:
    """In place: the gradient through the same mask (regenerated from (seed, key))."""
    _dev_check(G, key)
    assert G.dim() == 2 and G.shape[1] % 4 == 0
    with _rec("dropout", (G.shape[0], G.shape[1]), 8 * G.numel(), 0):
        H.check(H.lib().rl_dropout_bwd(G.data_ptr(), G.shape[0], first_row, G.shape[1], key.data_ptr(), seed & 0xFFFFFFFFFFFFFFFF, p,
                                       _st()), "rl_dropout_bwd")


def upsample_cf(feat: torch.Tensor, idx: torch.Tensor, d2: Optional[torch.Tensor], power: int) -> torch.Tensor:
    """feat (B,F,N1) channel-first, idx/d2 (B,N2,k) -> (B,F,N2)."""
    _dev_check(feat, idx, d2)
    B, Fc, N1 = feat.shape
    _, N2, k = idx.shape
    assert idx.dtype == torch.int32 and feat.dtype == F32 and idx.shape[0] == B
    out = torch.empty((B, Fc, N2), dtype=F32, device=feat.device)
    H.check(H.lib().rl_upsample_cf(feat.data_ptr(), idx.data_ptr(), H.ptr(d2), B, Fc, N1, N2, k, power,
                                   out.data_ptr(), _st()), "rl_upsample_cf")
    return out


def _perm_stride(perm: torch.Tensor, B: int, N: int) -> int:
    """0 for the reference's ONE permutation of a forward, N for one per cloud (band_sort)."""
    assert perm.dtype == torch.int64 and perm.is_contiguous() and perm.numel() in (N, B * N)
    return N if (perm.numel() == B * N and perm.dim() == 2) else 0


def logits_unpermute(lp: torch.Tensor, perm: torch.Tensor, B: int, N: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    Cc = lp.shape[1]
    assert lp.shape == (B * N, Cc)
    if out is None:
        out = torch.empty((B, Cc, N), dtype=F32, device=lp.device)
    else:
        _dev_check(out)
        assert out.shape == (B, Cc, N) and out.dtype == F32
    H.check(H.lib().rl_logits_unpermute_b(lp.data_ptr(), perm.data_ptr(), _perm_stride(perm, B, N), B, N, Cc, out.data_ptr(), _st()),
            "rl_logits_unpermute")
    return out


def logits_permute_grad(dlogits: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
    B, Cc, N = dlogits.shape
    _dev_check(dlogits, perm)
    out = torch.empty((B * N, Cc), dtype=F32, device=dlogits.device)
    H.check(H.lib().rl_logits_permute_grad_b(dlogits.data_ptr(), perm.data_ptr(), _perm_stride(perm, B, N), B, N, Cc, out.data_ptr(),
                                             _st()), "rl_logits_permute_grad")
    return out


NO_BAND_SORT = False      # test hook: the reference's permutation as drawn
BAND_SORT_MAX_BANDS = 8                                           # (bandsort.hip BS_MAXB: encoder levels + 1)


def band_sort(inp: torch.Tensor, perm: torch.Tensor, edges) -> torch.Tensor:
    """perm (N) -> (B, N): per cloud, the entries of every sampling band [edges[k], edges[k+1]) of the permutation ordered by
    the 4096-cell Morton code of the cloud's points (stable: ties keep the permutation's order).  The sampled SETS are the
    permutation's; the order inside them follows space (rl_band_sort).  inp: (B, N, 3 + F) fp32, x y z first."""
    _dev_check(inp, perm)
    B, N, cin = inp.shape
    assert inp.dtype == F32 and inp.is_contiguous() and perm.dtype == torch.int64 and perm.numel() == N
    e = (C.c_int * len(edges))(*[int(v) for v in edges])
    nb = len(edges) - 1
    need = H.lib().rl_band_sort_workspace_bytes(B, N, e, nb)
    if need < 0:
        H.check(-1, "rl_band_sort_workspace_bytes")
    ws = torch.empty(need, dtype=torch.uint8, device=inp.device)
    out = torch.empty((B, N), dtype=torch.int64, device=inp.device)
    with _rec("band_sort", (B, N), 40 * B * N, 0):
        H.check(H.lib().rl_band_sort(inp.data_ptr(), cin, perm.data_ptr(), B, N, e, nb, out.data_ptr(), ws.data_ptr(), need, _st()),
                "rl_band_sort")
    return out




# ------------------------------------------------------------------------------ loss, adam
REFERENCE_LOSSES = {  # reference trainer.py:244-269
    "cross_entropy": (0, 0.0, 0.0),
    "focal": (1, 0.0, 2.0),
    "dice": (2, 0.5, 1.0),
    "tversky": (2, 0.7, 1.0),
    "focal_tversky": (2, 0.7, 4.0 / 3.0),
}
SORTED_LOSSES = {  # no counterpart in the reference: the Lovasz-Softmax loss (utils/lovasz.py), alone and plus the masked cross entropy
    "lovasz": (3, 0.0, 0.0),
    "lovasz_cross_entropy": (4, 0.0, 0.0),
}


class _LossKinds:
    """name -> (kind, alpha, gamma).  Lookups (`[]`, `in`, get) know every loss; ITERATION (keys, items, values, len) walks the
    reference's losses only, as it always has: its users compare each entry with a value recorded from the reference
    (tests/golden/loss_metrics.npz), which has no sorted loss.  names() lists all of them."""

    def __getitem__(self, name):
        return REFERENCE_LOSSES[name] if name in REFERENCE_LOSSES else SORTED_LOSSES[name]

    def __contains__(self, name):
        return name in REFERENCE_LOSSES or name in SORTED_LOSSES

    def get(self, name, default=None):
        return self[name] if name in self else default

    def __iter__(self):
        return iter(REFERENCE_LOSSES)

    def __len__(self):
        return len(REFERENCE_LOSSES)

    def keys(self):
        return REFERENCE_LOSSES.keys()

    def items(self):
        return REFERENCE_LOSSES.items()

    def values(self):
        return REFERENCE_LOSSES.values()

    def names(self):
        return tuple(REFERENCE_LOSSES) + tuple(SORTED_LOSSES)


LOSS_KINDS = _LossKinds()
SORTED_KIND = 3     # kinds from here on are the sorted losses of csrc/lovasz.hip: always masked, never inside the fused head


def _masked_args(class_weights: Optional[torch.Tensor], ignore_unlabelled: bool, Cc: int, sync, who: str) -> bool:
    """The masked mode of the loss (include/rl_randlanet.h, rl_loss_forward_masked): class weights imply it.  Returns whether
    it is on; refuses what the kernels do not cover instead of computing something else."""
    masked = bool(ignore_unlabelled) or class_weights is not None
    if masked and sync is not None:
        raise H.HipKernelError(f"{who}: ignore_unlabelled / class_weights together with sync= (the data-parallel equivalence "
                               f"mode) is not supported: its global-batch kernels have no masked mode")
    if class_weights is not None:
        _dev_check(class_weights)
        assert class_weights.dtype == F32 and class_weights.numel() == Cc, f"{who}: class_weights must be {Cc} float32 values"
    return masked


def _sorted_args(kind: int, class_weights: Optional[torch.Tensor], Cc: int, sync, who: str) -> None:
    if kind not in (3, 4):
        raise H.HipKernelError(f"{who}: unknown loss kind {kind}")
    if sync is not None:
        raise H.HipKernelError(f"{who}: the Lovasz-Softmax loss together with sync= (the data-parallel equivalence mode) is "
                               f"not supported: its ranks are those of one sort over the whole batch")
    if class_weights is not None:
        _dev_check(class_weights)
        assert class_weights.dtype == F32 and class_weights.numel() == Cc, f"{who}: class_weights must be {Cc} float32 values"


def lovasz_workspace(device, B: int, Cc: int, N: int) -> torch.Tensor:
    """The workspace of rl_lovasz_forward / rl_lovasz_backward for (B, C, N) logits (uint8; torch allocations are 256-byte
    aligned).  Raises where the kernels refuse the sizes."""
    nbytes = H.lib().rl_lovasz_workspace_bytes(B, Cc, N)
    if nbytes < 0:
        raise H.HipKernelError(f"lovasz: B={B}, C={Cc}, N={N} is not supported: 1 .. {H.MAX_LOSS_CLASSES} classes and "
                               f"B*N*C < 2^31")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def lovasz_coef(work: torch.Tensor, B: int, Cc: int, N: int) -> torch.Tensor:
    """The (C, B*N) float32 coefficient table inside a workspace (a view)."""
    o = H.lib().rl_lovasz_coef_offset(B, Cc, N)
    return work[o:o + 4 * Cc * B * N].view(F32).view(Cc, B * N)


def _lovasz_forward(logits, labels, kind, out, sync, class_weights, work, return_coef):
    B, Cc, N = logits.shape
    _sorted_args(kind, class_weights, Cc, sync, "loss_forward")
    if work is None:
        work = lovasz_workspace(logits.device, B, Cc, N)
    else:
        _dev_check(work)
        assert work.dtype == torch.uint8 and work.numel() >= H.lib().rl_lovasz_workspace_bytes(B, Cc, N) >= 0
    if out is None:
        out = torch.empty(1 + 4 * Cc, dtype=torch.float64, device=logits.device)
    else:
        _dev_check(out)
        assert out.dtype == torch.float64 and out.numel() == 1 + 4 * Cc
    passes = -(-(32 + Cc.bit_length()) // 8)
    with _rec("loss", (B, Cc, N), (8 + 4 + passes * 32) * B * Cc * N + 8 * B * N, 0):
        H.check(H.lib().rl_lovasz_forward(logits.data_ptr(), labels.data_ptr(), B, Cc, N, int(kind == 4), H.ptr(class_weights),
                                          work.data_ptr(), work.numel(), out.data_ptr(), _st()), "rl_lovasz_forward")
    if return_coef:
        return out, work, lovasz_coef(work, B, Cc, N)
    return out, work


def loss_forward(logits: torch.Tensor, labels: torch.Tensor, kind: int, alpha: float, gamma: float,
                 neglect_background: bool = True, out: Optional[torch.Tensor] = None, sync: Optional[SyncGroup] = None,
                 class_weights: Optional[torch.Tensor] = None, ignore_unlabelled: bool = False,
                 work: Optional[torch.Tensor] = None, return_coef: bool = False):
    """Returns (out, work): out[0] = loss, out[1:] metric counts (doubles, on device).  With `sync` the class sums are
    all-reduced first: the loss (and the counts) of the GLOBAL batch, identical on every rank.
    ignore_unlabelled: points whose label is outside [0, C) add nothing to the loss or the counts; class_weights (C float32 on
    the device, checked by the caller - utils/losses.check_class_weights) weight the labelled ones and imply it.
    kind >= SORTED_KIND (lovasz, lovasz_cross_entropy): always the masked mode - with every label in range that is the default
    mode; `work` is the workspace of rl_lovasz_forward (lovasz_workspace; `work=` takes one made before, e.g. the static one
    of a captured step), alpha / gamma / neglect_background are not used, `sync` is refused.  return_coef: also the
    (C, B*N) float32 view of the workspace's coefficient table."""
    _dev_check(logits, labels)
    B, Cc, N = logits.shape
    assert labels.shape == (B, N) and labels.dtype == torch.int64 and logits.dtype == F32
    if kind >= SORTED_KIND:
        return _lovasz_forward(logits, labels, kind, out, sync, class_weights, work, return_coef)
    assert work is None and not return_coef, "work= / return_coef belong to the sorted losses"
    masked = _masked_args(class_weights, ignore_unlabelled, Cc, sync, "loss_forward")
    work = torch.empty(H.lib().rl_loss_work_doubles(B * N, Cc), dtype=torch.float64, device=logits.device)
    if out is None:
        out = torch.empty(1 + 4 * Cc, dtype=torch.float64, device=logits.device)
    else:
        _dev_check(out)
        assert out.dtype == torch.float64 and out.numel() == 1 + 4 * Cc
    if sync is not None:
        H.check(H.lib().rl_loss_partials(logits.data_ptr(), labels.data_ptr(), B, Cc, N, kind, gamma, work.data_ptr(), _st()),
                "rl_loss_partials")
        o = H.lib().rl_loss_totals_offset(Cc)
        sync.allreduce(work[o:o + 5 * Cc + 1])
        H.check(H.lib().rl_loss_from_totals(sync.global_rows(B * N), Cc, kind, alpha, gamma, int(neglect_background),
                                            work.data_ptr(), out.data_ptr(), _st()), "rl_loss_from_totals")
        return out, work
    with _rec("loss", (B, Cc, N), 4 * B * Cc * N + 8 * B * N, 0):
        if masked:
            H.check(H.lib().rl_loss_forward_masked(logits.data_ptr(), labels.data_ptr(), B, Cc, N, kind, alpha, gamma,
                                                   int(neglect_background), H.ptr(class_weights), 1, work.data_ptr(),
                                                   out.data_ptr(), _st()), "rl_loss_forward_masked")
        else:
            H.check(H.lib().rl_loss_forward(logits.data_ptr(), labels.data_ptr(), B, Cc, N, kind, alpha, gamma,
                                            int(neglect_background), work.data_ptr(), out.data_ptr(), _st()),
                    "rl_loss_forward")
    return out, work


def loss_backward(logits, labels, kind: int, alpha: float, gamma: float, neglect_background: bool, work,
                  grad_scale: float = 1.0, sync: Optional[SyncGroup] = None, class_weights: Optional[torch.Tensor] = None,
                  ignore_unlabelled: bool = False) -> torch.Tensor:
    """dloss/dlogits * grad_scale from the `work` of loss_forward; the same class_weights / ignore_unlabelled as there (an
    unlabelled point's gradient is exactly zero)."""
    B, Cc, N = logits.shape
    if kind >= SORTED_KIND:
        _sorted_args(kind, class_weights, Cc, sync, "loss_backward")
        dlogits = torch.empty_like(logits)
        with _rec("loss", (B, Cc, N), 12 * B * Cc * N + 8 * B * N, 0):
            H.check(H.lib().rl_lovasz_backward(logits.data_ptr(), labels.data_ptr(), B, Cc, N, int(kind == 4),
                                               H.ptr(class_weights), work.data_ptr(), work.numel(), grad_scale,
                                               dlogits.data_ptr(), _st()), "rl_lovasz_backward")
        return dlogits
    masked = _masked_args(class_weights, ignore_unlabelled, Cc, sync, "loss_backward")
    dlogits = torch.empty_like(logits)
    if sync is not None:
        H.check(H.lib().rl_loss_backward_global(logits.data_ptr(), labels.data_ptr(), B, Cc, N, kind, alpha, gamma,
                                                int(neglect_background), work.data_ptr(), grad_scale, sync.global_rows(B * N),
                                                dlogits.data_ptr(), _st()), "rl_loss_backward_global")
        return dlogits
    with _rec("loss", (B, Cc, N), 8 * B * Cc * N + 8 * B * N, 0):
        if masked:
            H.check(H.lib().rl_loss_backward_masked(logits.data_ptr(), labels.data_ptr(), B, Cc, N, kind, alpha, gamma,
                                                    int(neglect_background), work.data_ptr(), grad_scale,
                                                    H.ptr(class_weights), 1, dlogits.data_ptr(), _st()),
                    "rl_loss_backward_masked")
        else:
            H.check(H.lib().rl_loss_backward(logits.data_ptr(), labels.data_ptr(), B, Cc, N, kind, alpha, gamma,
                                             int(neglect_background), work.data_ptr(), grad_scale, dlogits.data_ptr(),
                                             _st()), "rl_loss_backward")
    return dlogits


class Head:
    """What the fused training step hands to Engine.forward so that the network's head - Dropout, fc_end.3, un-permute, loss and
    metric counts - runs as one kernel each way (rl_head_fwd / rl_head_bwd): the labels, the loss, where the step's record goes."""

    def __init__(self, labels: torch.Tensor, kind: int, alpha: float, gamma: float, neglect_background: bool, out: torch.Tensor,
                 grad_scale: float = 1.0, class_weights: Optional[torch.Tensor] = None, ignore_unlabelled: bool = False):
        self.labels, self.kind, self.alpha, self.gamma, self.neglect = labels, kind, alpha, gamma, neglect_background
        self.out, self.grad_scale = out, grad_scale
        self.class_weights, self.ignore_unlabelled = class_weights, ignore_unlabelled     # the loss' masked mode (loss_forward)
        self.work: Optional[torch.Tensor] = None
        self.mask: Optional[torch.Tensor] = None          # the rows' Dropout keep bits, forward -> backward


NO_FUSED_HEAD = False      # test hook: the separate launches


def head_supported(x: Lazy, Cc: int) -> bool:
    return (not NO_FUSED_HEAD and x.C == 32 and x.raw.dtype == F32 and x.raw.shape[1] == 32 and x.bstride == x.n
            and bool(H.lib().rl_head_supported(Cc, 32)))


def _head_desc(x: Lazy, W: torch.Tensor, bias: torch.Tensor, perm: torch.Tensor, head: Head, drop) -> "H.HeadDesc":
    _dev_check(x.raw, W, bias, perm, head.labels, head.out, x.scale, x.shift, x.mean, x.invstd)
    B, N, Cc = x.B, x.n, W.shape[0]
    assert W.dtype == F32 and W.numel() == Cc * 32 and bias.numel() == Cc
    assert head.labels.shape == (B, N) and head.labels.dtype == torch.int64 and head.out.numel() == 1 + 4 * Cc
    d = H.HeadDesc()
    d.X, d.scale, d.shift, d.act, d.slope = x.raw.data_ptr(), H.ptr(x.scale), H.ptr(x.shift), x.act, x.slope
    d.mean, d.invstd = H.ptr(x.mean), H.ptr(x.invstd)
    d.W, d.bias, d.perm, d.labels = W.data_ptr(), bias.data_ptr(), perm.data_ptr(), head.labels.data_ptr()
    d.perm_bstride = _perm_stride(perm, x.B, N)
    d.B, d.N, d.C = B, N, Cc
    d.loss_kind, d.alpha, d.gamma, d.neglect_background = head.kind, head.alpha, head.gamma, int(head.neglect)
    key, seed, p_drop, first_row = drop
    d.drop_p, d.drop_key, d.drop_seed, d.drop_first_row = (p_drop if key is not None else 0.0), H.ptr(key), seed, first_row
    d.grad_scale = head.grad_scale
    d.masked = int(_masked_args(head.class_weights, head.ignore_unlabelled, Cc, None, "head"))
    d.class_weight = H.ptr(head.class_weights)
    return d


def head_fwd(x: Lazy, W: torch.Tensor, bias: torch.Tensor, perm: torch.Tensor, head: Head, drop) -> None:
    """Dropout -> fc_end.3 -> un-permute -> loss + counts of the rows of `x` (fc_end.1's lazy output, permuted order) in one
    launch + the loss finalize: fills head.out (rl_loss_forward's record) and head.work.  drop = (key, seed, p, first_row)."""
    d = _head_desc(x, W, bias, perm, head, drop)
    head.work = torch.empty(H.lib().rl_loss_work_doubles(x.rows, d.C), dtype=torch.float64, device=W.device)
    d.work = head.work.data_ptr()
    if d.drop_p > 0.0:
        head.mask = torch.empty(x.rows, dtype=torch.int32, device=W.device)
        d.drop_mask = head.mask.data_ptr()
    with _rec("head_fwd", (x.rows, 32, d.C), 4 * x.rows * 32 + 16 * x.rows, 2 * x.rows * 32 * d.C):
        H.check(H.lib().rl_head_fwd(C.byref(d), head.out.data_ptr(), _st()), "rl_head_fwd")


def head_bwd(x: Lazy, W: torch.Tensor, bias: torch.Tensor, perm: torch.Tensor, head: Head, drop, dW: torch.Tensor,
             dbias: torch.Tensor, pending: list):
    """The whole backward of the head: returns (G, (bn_bwd_partials, nslots)) - G the gradient w.r.t. x's ACTIVATED value, the
    partials what rl_bn_bwd_reduce would leave for x's BatchNorm; fc_end.3's weight / bias gradient slabs join `pending`."""
    d = _head_desc(x, W, bias, perm, head, drop)
    Cc = d.C
    d.work = head.work.data_ptr()
    g = H.lib().rl_head_grid(x.rows)
    G = torch.empty((x.rows, 32), dtype=F32, device=W.device)
    slab = torch.empty(g * (Cc * 32 + Cc), dtype=F32, device=W.device)
    bstats = torch.empty((g, 2, 32), dtype=torch.float64, device=W.device) if x.mean is not None else None
    d.G, d.slab, d.slab_floats, d.bn_bwd_stats = G.data_ptr(), slab.data_ptr(), slab.numel(), H.ptr(bstats)
    d.drop_mask = H.ptr(head.mask)
    with _rec("head_bwd", (x.rows, 32, Cc), 8 * x.rows * 32 + 16 * x.rows, 4 * x.rows * 32 * Cc):
        H.check(H.lib().rl_head_bwd(C.byref(d), _st()), "rl_head_bwd")
    it = H.WgradReduceItem()
    it.slab, it.dW, it.dbias, it.w_ks, it.w_ns = slab.data_ptr(), dW.data_ptr(), dbias.data_ptr(), 1, 32
    it.nsplit, it.N, it.K = g, Cc, 32
    pending.append((it, slab, dW, dbias))
    return G, ((bstats, g) if bstats is not None else None)


def softmax_cf(logits: torch.Tensor) -> torch.Tensor:
    """Softmax over dim 1 of (B,C,N) logits."""
    _dev_check(logits)
    assert logits.dim() == 3 and logits.dtype == F32
    B, Cc, N = logits.shape
    out = torch.empty_like(logits)
    H.check(H.lib().rl_softmax_cf(logits.data_ptr(), B, Cc, N, out.data_ptr(), _st()), "rl_softmax_cf")
    return out


def adam_step(param, grad, exp_avg, exp_avg_sq, lr: torch.Tensor, step: torch.Tensor, beta1=0.9, beta2=0.999,
              eps=1e-8, grad_scale=1.0) -> None:
    _dev_check(param, grad, exp_avg, exp_avg_sq, lr, step)
    n = param.numel()
    assert grad.numel() == n and exp_avg.numel() == n and exp_avg_sq.numel() == n
    assert lr.dtype == F32 and step.dtype == torch.int64
    with _rec("adam", (n,), 28 * n, 0):
        H.check(H.lib().rl_adam_step(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), n,
                                     lr.data_ptr(), beta1, beta2, eps, grad_scale, step.data_ptr(), _st()),
                "rl_adam_step")


# ------------------------------------------------------------------------------------------ voted-crop scene inference
def _workspace(symbol: str, device, *sizes) -> torch.Tensor:
    """Device scratch of `symbol`'s size (an rl_*_workspace_bytes of the library) for `sizes`."""
    return torch.empty(int(getattr(H.lib(), symbol)(*sizes)), dtype=torch.uint8, device=device)


def scene_workspace(device, M: int, n: int) -> torch.Tensor:
    """Device scratch of rl_scene_crop / rl_scene_min_count (256-byte aligned: torch's allocator aligns to 512)."""
    return _workspace("rl_scene_workspace_bytes", device, M, n)


def scene_crop(cloud: torch.Tensor, possibility: torch.Tensor, n: int, rows_out: torch.Tensor, idx_out: torch.Tensor,
               ws: torch.Tensor, pad: bool = False) -> None:
    """One crop: pick the least covered point, write the n nearest points (ascending index) to idx_out (n) int32 and their
    cloud rows to rows_out (n, >= dim), raise their possibilities.  rows_out / idx_out may be rows of larger tensors.
    pad: rl_scene_crop_padded - n may exceed M; the cloud is then taken whole and repeated cyclically over the n slots."""
    _dev_check(cloud, possibility, ws)
    M, dim = cloud.shape
    assert cloud.dtype == F32 and possibility.dtype == F32 and possibility.shape == (M,)
    assert rows_out.dtype == F32 and rows_out.is_cuda and rows_out.dim() == 2 and rows_out.shape[0] >= n
    assert rows_out.shape[1] >= dim and rows_out.stride(1) == 1
    assert idx_out.dtype == torch.int32 and idx_out.is_contiguous() and idx_out.numel() >= n
    assert rows_out.get_device() == idx_out.get_device() == cloud.get_device()
    name = "rl_scene_crop_padded" if pad else "rl_scene_crop"
    H.check(getattr(H.lib(), name)(cloud.data_ptr(), M, dim, possibility.data_ptr(), n, rows_out.data_ptr(),
                                   rows_out.stride(0), idx_out.data_ptr(), ws.data_ptr(), ws.numel(), _st()), name)


def scene_accumulate(logits: torch.Tensor, idx: torch.Tensor, one_minus_s: float, s: float, prob: torch.Tensor,
                     count: torch.Tensor, first: Optional[int] = None) -> None:
    """prob (M, C) <- s*prob + (1-s)*softmax(logits (C, n)) at the crop's points idx (n), count += 1 there.
    first: rl_scene_accumulate_first - only the first `first` slots of the crop (the class stride of logits may exceed n);
    the other slots leave prob and count untouched."""
    # (with `first` the logits may be the leading columns of wider rows: checked below instead of for contiguity)
    _dev_check(logits if first is None else logits.new_empty(0), idx, prob, count)
    Cc, n = logits.shape
    M = prob.shape[0]
    assert logits.dtype == F32 and idx.dtype == torch.int32 and idx.numel() == n
    assert prob.dtype == F32 and prob.shape == (M, Cc) and count.dtype == torch.int32 and count.shape == (M,)
    if first is None:
        H.check(H.lib().rl_scene_accumulate(logits.data_ptr(), Cc, n, idx.data_ptr(), one_minus_s, s, prob.data_ptr(),
                                            count.data_ptr(), M, _st()), "rl_scene_accumulate")
        return
    assert logits.stride(1) == 1 and (Cc == 1 or logits.stride(0) >= n) and idx.is_contiguous()
    ld = logits.stride(0) if Cc > 1 else n
    H.check(H.lib().rl_scene_accumulate_first(logits.data_ptr(), Cc, n, idx.data_ptr(), one_minus_s, s, prob.data_ptr(),
                                              count.data_ptr(), M, ld, first, _st()), "rl_scene_accumulate_first")


def scene_min_count(count: torch.Tensor, out: torch.Tensor, ws: torch.Tensor) -> None:
    """out[0] = min(count), on the device."""
    _dev_check(count, out, ws)
    assert count.dtype == torch.int32 and out.dtype == torch.int32 and out.numel() >= 1
    H.check(H.lib().rl_scene_min_count(count.data_ptr(), count.numel(), out.data_ptr(), ws.data_ptr(), _st()),
            "rl_scene_min_count")


# ------------------------------------------------------------------------------------------ training crops over many scenes
def scenes_workspace(device, S: int, max_points: int, n: int) -> torch.Tensor:
    """Device scratch of rl_scenes_init / rl_scenes_crop (256-byte aligned: torch's allocator aligns to 512)."""
    return _workspace("rl_scenes_workspace_bytes", device, S, max_points, n)


def scenes_init(off: torch.Tensor, possibility: torch.Tensor, ws: torch.Tensor, max_points: int) -> None:
    """The per-scene state of rl_scenes_crop from the current possibilities; off (S+1) int64 on the device."""
    _dev_check(off, possibility, ws)
    assert off.dtype == torch.int64 and off.is_contiguous() and off.numel() >= 2
    assert possibility.dtype == F32 and possibility.is_contiguous()
    H.check(H.lib().rl_scenes_init(off.data_ptr(), off.numel() - 1, max_points, possibility.data_ptr(), ws.data_ptr(),
                                   ws.numel(), _st()), "rl_scenes_init")


def scenes_crop(xyz: torch.Tensor, possibility: torch.Tensor, n: int, idx_out: torch.Tensor, scene_out: torch.Tensor,
                ws: torch.Tensor, S: int, max_points: int, noise: Optional[torch.Tensor] = None,
                pad: bool = False) -> None:
    """B = scene_out.numel() crops in order: global rows (B, n) int64 into idx_out, scene ids (B) int64 into scene_out, the
    possibilities raised; noise (B, 3) float32 offsets the centres.  ws prepared by scenes_init.
    pad: rl_scenes_crop_padded - a picked scene of fewer than n points is taken whole and repeated cyclically."""
    _dev_check(xyz, possibility, ws, idx_out, scene_out)
    B = scene_out.numel()
    assert xyz.dtype == F32 and xyz.dim() == 2 and xyz.shape[1] >= 3 and xyz.stride(1) == 1
    assert possibility.dtype == F32 and possibility.is_contiguous() and possibility.shape == (xyz.shape[0],)
    assert idx_out.dtype == torch.int64 and idx_out.is_contiguous() and idx_out.numel() == B * n
    assert scene_out.dtype == torch.int64 and scene_out.is_contiguous()
    if noise is not None:
        _dev_check(noise)
        assert noise.dtype == F32 and noise.is_contiguous() and noise.numel() == 3 * B
    name = "rl_scenes_crop_padded" if pad else "rl_scenes_crop"
    H.check(getattr(H.lib(), name)(xyz.data_ptr(), xyz.stride(0), S, max_points, possibility.data_ptr(), n, B,
                                   H.ptr(noise), idx_out.data_ptr(), scene_out.data_ptr(), ws.data_ptr(), ws.numel(),
                                   _st()), name)


# ------------------------------------------------------------------------------------------ voted crops over many scenes
def scenes_vote_crop(cloud: torch.Tensor, possibility: torch.Tensor, count: torch.Tensor, low: torch.Tensor, votes: int,
                     n: int, rows_out: torch.Tensor, idx_out: torch.Tensor, scene_out: torch.Tensor,
                     first_out: torch.Tensor, open_out: torch.Tensor, ws: torch.Tensor, S: int, max_points: int,
                     pad: bool = False) -> None:
    """B = scene_out.numel() vote crops in order over cloud (T, dim): every slot goes to the least covered point among the
    scenes whose least count (low (S) int32) is below `votes`; global rows (B, n) int64 into idx_out, the cloud rows into
    rows_out (B, n, >= dim), scene ids (B) int64 (-1: an idle slot, whose idx_out / rows_out keep what they hold) into
    scene_out, the duplicate-free leading slots (B) int32 into first_out, the open scenes left into open_out (1) int32;
    possibility, count (T) int32 and low raised.  count and low start zeroed; ws prepared by scenes_init."""
    _dev_check(cloud, possibility, count, low, ws, idx_out, scene_out, first_out, open_out, rows_out.new_empty(0))
    B = scene_out.numel()
    T, dim = cloud.shape
    assert cloud.dtype == F32 and cloud.is_contiguous() and dim >= 3
    assert possibility.dtype == F32 and possibility.is_contiguous() and possibility.shape == (T,)
    assert count.dtype == torch.int32 and count.is_contiguous() and count.shape == (T,)
    assert low.dtype == torch.int32 and low.is_contiguous() and low.shape == (S,)
    assert rows_out.dtype == F32 and rows_out.is_cuda and rows_out.shape[:2] == (B, n) and rows_out.shape[2] >= dim
    assert rows_out.stride(2) == 1 and rows_out.get_device() == cloud.get_device()
    assert idx_out.dtype == torch.int64 and idx_out.is_contiguous() and idx_out.numel() == B * n
    assert scene_out.dtype == torch.int64 and scene_out.is_contiguous()
    assert first_out.dtype == torch.int32 and first_out.is_contiguous() and first_out.numel() == B
    assert open_out.dtype == torch.int32 and open_out.numel() >= 1
    H.check(H.lib().rl_scenes_vote_crop(cloud.data_ptr(), dim, S, max_points, possibility.data_ptr(), count.data_ptr(),
                                        low.data_ptr(), votes, n, B, 1 if pad else 0, rows_out.data_ptr(),
                                        rows_out.stride(0), rows_out.stride(1), idx_out.data_ptr(), scene_out.data_ptr(),
                                        first_out.data_ptr(), open_out.data_ptr(), ws.data_ptr(), ws.numel(), _st()),
            "rl_scenes_vote_crop")


def scenes_vote_accumulate(logits: torch.Tensor, idx: torch.Tensor, first: torch.Tensor, one_minus_s: float, s: float,
                           prob: torch.Tensor) -> None:
    """prob (T, C) <- s*prob + (1-s)*softmax(logits[b] (C, n)) at the global rows idx[b, :first[b]], slot after slot in
    order; first (B) int32 stays on the device (scenes_vote_crop's first_out: 0 for an idle slot).  No count changes."""
    # (the logits may be the leading columns of wider rows: their strides are checked below instead of for contiguity)
    _dev_check(logits.new_empty(0), idx, first, prob)
    B, Cc, n = logits.shape
    T = prob.shape[0]
    assert logits.dtype == F32 and logits.stride(2) == 1 and (Cc == 1 or logits.stride(1) >= n)
    assert idx.dtype == torch.int64 and idx.shape == (B, n)
    assert first.dtype == torch.int32 and first.numel() == B
    assert prob.dtype == F32 and prob.shape == (T, Cc)
    ld = logits.stride(1) if Cc > 1 else n
    H.check(H.lib().rl_scenes_vote_accumulate(logits.data_ptr(), Cc, n, ld, logits.stride(0), B, idx.data_ptr(),
                                              first.data_ptr(), one_minus_s, s, prob.data_ptr(), T, _st()),
            "rl_scenes_vote_accumulate")


# ------------------------------------------------------------------------------------------ grid subsampling, scene scoring
def grid_workspace(device, M: int, dim: int) -> torch.Tensor:
    """Device scratch of rl_grid_bounds / rl_grid_sort / rl_grid_heads / rl_grid_reduce (256-byte aligned: torch's allocator aligns to 512)."""
    return _workspace("rl_grid_workspace_bytes", device, M, dim)


def grid_subsample(cloud: torch.Tensor, labels: Optional[torch.Tensor], cell: float, n_classes: Optional[int] = None):
    """One representative per occupied voxel of edge `cell` of cloud (M, dim) float32 (finite coordinates; labels (M) int64
    or None - the caller checked on the host that they are inside [0, n_classes) unless it allows unlabelled points: a label
    outside the range does not vote, and a cell without a vote gets -1).  Returns device tensors (rows (V, dim) float32,
    labels (V) int64 or None, inverse (M) int32, count (V) int32), the bits of utils/grid.py's grid_subsample_host.  Two
    read-backs: the grid dimensions (ValueError when one reaches 2^21) and V."""
    from .utils import grid as G
    _dev_check(cloud, labels)
    M, dim = cloud.shape
    assert cloud.dtype == F32 and cloud.is_contiguous() and dim >= 3
    if labels is not None:
        assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.shape == (M,)
        assert n_classes is not None and int(n_classes) > 0, "labels given without n_classes"
    dev = cloud.device
    lib = H.lib()
    ws = grid_workspace(dev, M, dim)
    head = torch.empty(4, dtype=torch.int64, device=dev)          # dims x, y, z and V
    H.check(lib.rl_grid_bounds(cloud.data_ptr(), M, dim, cell, head.data_ptr(), ws.data_ptr(), ws.numel(), _st()),
            "rl_grid_bounds")
    dims = head[:3].tolist()                                       # read-back 1
    G.check_dims(dims)
    inverse = torch.empty(M, dtype=torch.int32, device=dev)
    H.check(lib.rl_grid_sort(cloud.data_ptr(), M, dim, G.key_bits(dims), ws.data_ptr(), ws.numel(), _st()), "rl_grid_sort")
    H.check(lib.rl_grid_heads(M, dim, head[3:].data_ptr(), inverse.data_ptr(), ws.data_ptr(), ws.numel(), _st()),
            "rl_grid_heads")
    V = int(head[3].item())                                        # read-back 2
    rows = torch.empty((V, dim), dtype=F32, device=dev)
    count = torch.empty(V, dtype=torch.int32, device=dev)
    lab = torch.empty(V, dtype=torch.int64, device=dev) if labels is not None else None
    H.check(lib.rl_grid_reduce(cloud.data_ptr(), M, dim, H.ptr(labels), int(n_classes) if labels is not None else 0, V,
                               rows.data_ptr(), H.ptr(lab), count.data_ptr(), ws.data_ptr(), ws.numel(), _st()),
            "rl_grid_reduce")
    return rows, lab, inverse, count


def scene_confusion(prob: torch.Tensor, labels: torch.Tensor, table: torch.Tensor,
                    inverse: Optional[torch.Tensor] = None) -> None:
    """table (C, C) int64 += the confusion counts of labels (M) int64 against the argmax of prob (V, C) rows inverse (M)
    int32 (or the point's own row); labels outside [0, C) are skipped."""
    _dev_check(prob, labels, table, inverse)
    V, Cc = prob.shape
    M = labels.numel()
    assert prob.dtype == F32 and prob.is_contiguous() and labels.dtype == torch.int64 and labels.is_contiguous()
    assert table.dtype == torch.int64 and table.is_contiguous() and table.shape == (Cc, Cc)
    if inverse is not None:
        assert inverse.dtype == torch.int32 and inverse.is_contiguous() and inverse.numel() == M
    H.check(H.lib().rl_scene_confusion(prob.data_ptr(), V, Cc, labels.data_ptr(), M, H.ptr(inverse), table.data_ptr(),
                                       _st()), "rl_scene_confusion")


# ------------------------------------------------------------------------------------------ instances of a labelled scene
def cluster_workspace(device, M: int) -> torch.Tensor:
    """Device scratch of rl_cluster_cells / rl_cluster_union / rl_cluster_reduce (256-byte aligned: torch's allocator aligns to 512)."""
    return _workspace("rl_cluster_workspace_bytes", device, M)


def euclidean_clusters(xyz: torch.Tensor, labels: torch.Tensor, radius: float, min_points: int = 1, ignore=(0,),
                       scores: Optional[torch.Tensor] = None, min_samples: int = 1):
    """The instances of xyz (M, 3) float32 (finite coordinates: the caller checked on the host) under labels (M) int64: the
    components of the points that take part (label >= 0, not in `ignore`) joined within `radius` inside a label, those below
    min_points dropped, the others numbered by their smallest point.  Returns device tensors (instance (M) int32, classes (I)
    int64, count (I) int32, centroid (I, 3), lo (I, 3), hi (I, 3) float32, score (I) float32 or None without scores (M)
    float32), the bits of utils/cluster.py's euclidean_clusters_host.  Two read-backs: the grid dimensions (ValueError when
    one reaches 2^16) and I.  min_samples above 1: the density rule (rl_cluster_union_dense; utils/cluster.py, "density"),
    the same read-backs; 1 launches what it always launched."""
    return _clusters(xyz, labels, radius, min_points, ignore, scores, None, min_samples)


def _grown_workspace(cache: dict, symbol: str, device, *sizes) -> torch.Tensor:
    """The workspace `cache` keeps for the device, kept from call to call (a scene after a scene reuses it) and made anew only
    when the library's `symbol`(*sizes) asks for more bytes than it has."""
    nbytes = int(getattr(H.lib(), symbol)(*sizes))
    key = torch.device(device)
    key = (key.type, torch.cuda.current_device() if key.index is None else key.index)
    ws = cache.get(key)
    if ws is None or ws.numel() < nbytes:
        cache[key] = None                                          # (the old one is freed before the new one is made)
        ws = cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


_smooth_ws, _dense_ws = {}, {}      # device -> the smooth rule's and the density rule's workspace


def smooth_cluster_workspace(device, M: int) -> torch.Tensor:
    """Device scratch of rl_cluster_cells / rl_cluster_union_smooth / rl_cluster_reduce: cluster_workspace's, then the packed
    normals.  Cached per device; only a larger cloud allocates again."""
    return _grown_workspace(_smooth_ws, "rl_cluster_smooth_workspace_bytes", device, M)


def dense_cluster_workspace(device, M: int, smooth: bool) -> torch.Tensor:
    """Device scratch of rl_cluster_cells / rl_cluster_union_dense / rl_cluster_reduce: the workspace of the rule it extends,
    then support and attach.  Cached per device; only a cloud that needs more allocates again."""
    return _grown_workspace(_dense_ws, "rl_cluster_dense_workspace_bytes", device, M, 1 if smooth else 0)


def smooth_clusters(xyz: torch.Tensor, labels: torch.Tensor, radius: float, normals: torch.Tensor, cos_angle: float,
                    min_points: int = 1, ignore=(0,), scores: Optional[torch.Tensor] = None,
                    curvature: Optional[torch.Tensor] = None, max_curvature: Optional[float] = None, min_samples: int = 1):
    """euclidean_clusters under the smooth rule (rl_cluster_union_smooth): an edge needs, besides, abs(n_i . n_j) >= cos_angle
    - the caller's float32(cos(normal_angle)) - for the normals (M, 3) float32 (finite: the caller checked on the host), and
    with curvature (M) float32 and max_curvature a point above float32(max_curvature) takes no part.  The same seven device
    tensors, the bits of euclidean_clusters_host(normals=..., normal_angle=...), the same two read-backs.  min_samples as in
    euclidean_clusters: support counts the plain rule, the edges between core points are the smooth ones."""
    M = xyz.shape[0]
    _dev_check(normals, curvature)
    assert normals.dtype == F32 and normals.is_contiguous() and normals.shape == (M, 3)
    assert (curvature is None) == (max_curvature is None), "curvature and max_curvature go together"
    if curvature is not None:
        assert curvature.dtype == F32 and curvature.is_contiguous() and curvature.shape == (M,)
    return _clusters(xyz, labels, radius, min_points, ignore, scores,
                     (normals, curvature, float(cos_angle), float(max_curvature) if curvature is not None else 0.0), min_samples)


def _clusters(xyz, labels, radius, min_points, ignore, scores, smooth, min_samples=1):
    """euclidean_clusters (smooth None) and smooth_clusters (smooth = (normals, curvature or None, cos_angle, max_curvature)).
    min_samples == 1 calls the entries of the two rules, the launches they always made; anything else rl_cluster_union_dense."""
    from .utils import cluster as K
    _dev_check(xyz, labels, scores)
    M = xyz.shape[0]
    assert xyz.dtype == F32 and xyz.is_contiguous() and xyz.shape == (M, 3)
    assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.shape == (M,)
    if scores is not None:
        assert scores.dtype == F32 and scores.is_contiguous() and scores.shape == (M,)
    dev = xyz.device
    lib = H.lib()
    ign = torch.tensor([int(c) for c in ignore], dtype=torch.int64).to(dev)
    if int(min_samples) != min_samples or int(min_samples) < 1:
        raise ValueError(f"euclidean_clusters: min_samples={min_samples!r} must be an integer >= 1")
    dense = int(min_samples) != 1
    if dense:
        ws = dense_cluster_workspace(dev, M, smooth is not None)
    else:
        ws = cluster_workspace(dev, M) if smooth is None else smooth_cluster_workspace(dev, M)
    head = torch.empty(4, dtype=torch.int64, device=dev)          # dims x, y, z and I
    H.check(lib.rl_cluster_cells(xyz.data_ptr(), M, radius, head.data_ptr(), ws.data_ptr(), ws.numel(), _st()),
            "rl_cluster_cells")
    dims = head[:3].tolist()                                       # read-back 1
    K.check_dims(dims)
    instance = torch.empty(M, dtype=torch.int32, device=dev)
    if dense:
        normals, curvature, cos_angle, max_curvature = smooth if smooth is not None else (None, None, 0.0, 0.0)
        H.check(lib.rl_cluster_union_dense(xyz.data_ptr(), labels.data_ptr(), M, radius,
                                           ign.data_ptr() if ign.numel() else None, ign.numel(), K.key_bits(dims),
                                           int(min_points), H.ptr(normals), H.ptr(curvature), cos_angle, max_curvature,
                                           int(min_samples), instance.data_ptr(), head[3:].data_ptr(), ws.data_ptr(), ws.numel(),
                                           _st()), "rl_cluster_union_dense")
    elif smooth is None:
        H.check(lib.rl_cluster_union(xyz.data_ptr(), labels.data_ptr(), M, radius, ign.data_ptr() if ign.numel() else None,
                                     ign.numel(), K.key_bits(dims), int(min_points), instance.data_ptr(),
                                     head[3:].data_ptr(), ws.data_ptr(), ws.numel(), _st()), "rl_cluster_union")
    else:
        normals, curvature, cos_angle, max_curvature = smooth
        H.check(lib.rl_cluster_union_smooth(xyz.data_ptr(), labels.data_ptr(), M, radius,
                                            ign.data_ptr() if ign.numel() else None, ign.numel(), K.key_bits(dims),
                                            int(min_points), normals.data_ptr(), H.ptr(curvature), cos_angle, max_curvature,
                                            instance.data_ptr(), head[3:].data_ptr(), ws.data_ptr(), ws.numel(), _st()),
                "rl_cluster_union_smooth")
    I = int(head[3].item())                                        # read-back 2
    classes = torch.empty(I, dtype=torch.int64, device=dev)
    count = torch.empty(I, dtype=torch.int32, device=dev)
    centroid, lo, hi = (torch.empty((I, 3), dtype=F32, device=dev) for _ in range(3))
    score = torch.empty(I, dtype=F32, device=dev) if scores is not None else None
    if I > 0:
        H.check(lib.rl_cluster_reduce(xyz.data_ptr(), labels.data_ptr(), H.ptr(scores), M, I, classes.data_ptr(),
                                      count.data_ptr(), centroid.data_ptr(), lo.data_ptr(), hi.data_ptr(), H.ptr(score),
                                      ws.data_ptr(), ws.numel(), _st()), "rl_cluster_reduce")
    return instance, classes, count, centroid, lo, hi, score


def scene_labels(prob: torch.Tensor, min_confidence: float = 0.0):
    """(labels (V) int64, confidence (V) float32) of prob (V, C) float32: the argmax of every row (ties to the lowest class),
    its share of the row's sum, and -1 for the label where that share is below min_confidence."""
    _dev_check(prob)
    V, Cc = prob.shape
    assert prob.dtype == F32 and prob.is_contiguous()
    labels = torch.empty(V, dtype=torch.int64, device=prob.device)
    conf = torch.empty(V, dtype=F32, device=prob.device)
    H.check(H.lib().rl_scene_labels(prob.data_ptr(), V, Cc, float(min_confidence), labels.data_ptr(), conf.data_ptr(), _st()),
            "rl_scene_labels")
    return labels, conf


# ------------------------------------------------------------------------------------------ keypoints of a scored scene
def keypoints_workspace(device, M: int) -> torch.Tensor:
    """Device scratch of rl_keypoints_* (256-byte aligned: torch's allocator aligns to 512)."""
    return _workspace("rl_keypoints_workspace_bytes", device, M)


def confidence_peaks(xyz: torch.Tensor, labels: torch.Tensor, scores: torch.Tensor, radius: float, min_score: float = 0.0,
                     min_points: int = 1, ignore=(0,)):
    """The keypoints of xyz (M, 3) float32 under labels (M) int64 and scores (M) float32 (finite coordinates, finite scores >=
    0: the caller checked on the host): the live points - label >= 0, not in `ignore`, score >= min_score, at least min_points
    such points of their label within `radius` - that no live point of their label within `radius` beats, each with the
    score-weighted mean of the live points around it.  Returns device tensors (index (K) int64, classes (K) int64, position
    (K, 3), score (K), mean_score (K) float32, count (K) int32), the bits of utils/keypoints.py's confidence_peaks_host.  Two
    read-backs: the grid dimensions (ValueError when one reaches 2^16) and K."""
    from .utils import cluster as K
    _dev_check(xyz, labels, scores)
    M = xyz.shape[0]
    assert xyz.dtype == F32 and xyz.is_contiguous() and xyz.shape == (M, 3)
    assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.shape == (M,)
    assert scores.dtype == F32 and scores.is_contiguous() and scores.shape == (M,)
    dev = xyz.device
    lib = H.lib()
    ign = torch.tensor([int(c) for c in ignore], dtype=torch.int64).to(dev)
    ws = keypoints_workspace(dev, M)
    wsp, wsn = ws.data_ptr(), ws.numel()
    head = torch.empty(4, dtype=torch.int64, device=dev)          # dims x, y, z and K
    H.check(lib.rl_keypoints_cells(xyz.data_ptr(), M, radius, head.data_ptr(), wsp, wsn, _st()), "rl_keypoints_cells")
    dims = head[:3].tolist()                                       # read-back 1
    K.check_dims(dims)
    H.check(lib.rl_keypoints_sort(xyz.data_ptr(), labels.data_ptr(), scores.data_ptr(), M, float(min_score),
                                  ign.data_ptr() if ign.numel() else None, ign.numel(), K.key_bits(dims), wsp, wsn, _st()),
            "rl_keypoints_sort")
    H.check(lib.rl_keypoints_support(labels.data_ptr(), M, radius, wsp, wsn, _st()), "rl_keypoints_support")
    H.check(lib.rl_keypoints_peaks(labels.data_ptr(), M, radius, int(min_points), head[3:].data_ptr(), wsp, wsn, _st()),
            "rl_keypoints_peaks")
    n = int(head[3].item())                                        # read-back 2
    index = torch.empty(n, dtype=torch.int64, device=dev)
    classes = torch.empty(n, dtype=torch.int64, device=dev)
    position = torch.empty((n, 3), dtype=F32, device=dev)
    score, mean = torch.empty(n, dtype=F32, device=dev), torch.empty(n, dtype=F32, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    if n > 0:
        H.check(lib.rl_keypoints_refine(labels.data_ptr(), M, n, radius, int(min_points), index.data_ptr(), classes.data_ptr(),
                                        position.data_ptr(), score.data_ptr(), mean.data_ptr(), count.data_ptr(), wsp, wsn,
                                        _st()), "rl_keypoints_refine")
    return index, classes, position, score, mean, count


# ------------------------------------------------------------------------------------------- pair counts of two id arrays
def pairs_workspace(device, M: int) -> torch.Tensor:
    """Device scratch of rl_pairs_sort / rl_pairs_write (256-byte aligned: torch's allocator aligns to 512)."""
    return _workspace("rl_pairs_workspace_bytes", device, M)


def pair_counts(a: torch.Tensor, b: torch.Tensor, A: int, B: int):
    """The pairs (a_i, b_i) that occur among a, b (M) int32 or int64 (1 <= A, B <= 2^31 - 1: the caller checked on the host;
    values below -1 count as -1), in ascending order of (a, b) with -1 first.  Returns device tensors (pa (P) int32, pb (P)
    int32, count (P) int64), the arrays of utils/instance_metrics.py's pair_counts_host.  One read-back: P together with the
    flag of a value >= A or >= B (ValueError)."""
    from .utils import instance_metrics as IM
    _dev_check(a, b)
    M = a.numel()
    assert a.shape == (M,) and b.shape == (M,)
    assert a.dtype in (torch.int32, torch.int64) and b.dtype in (torch.int32, torch.int64)
    dev = a.device
    lib = H.lib()
    ws = pairs_workspace(dev, M)
    head = torch.empty(2, dtype=torch.int64, device=dev)          # P and the flag
    H.check(lib.rl_pairs_sort(a.data_ptr(), a.element_size(), b.data_ptr(), b.element_size(), M, int(A), int(B),
                              head.data_ptr(), ws.data_ptr(), ws.numel(), _st()), "rl_pairs_sort")
    P, flag = head.tolist()                                        # the read-back
    if flag:
        raise IM.out_of_range(int(A), int(B))
    pa = torch.empty(P, dtype=torch.int32, device=dev)
    pb = torch.empty(P, dtype=torch.int32, device=dev)
    count = torch.empty(P, dtype=torch.int64, device=dev)
    H.check(lib.rl_pairs_write(M, int(A), int(B), P, pa.data_ptr(), pb.data_ptr(), count.data_ptr(), ws.data_ptr(),
                               ws.numel(), _st()), "rl_pairs_write")
    return pa, pb, count


# --------------------------------------------------------------------------------------- oriented boxes of point sets by id
def boxes_workspace(device, M: int, I: int) -> torch.Tensor:
    """Device scratch of rl_boxes_sort / rl_boxes_moments / rl_boxes_fit (256-byte aligned: torch's allocator aligns to 512)."""
    return _workspace("rl_boxes_workspace_bytes", device, M, I)


def instance_boxes(xyz: torch.Tensor, ids: torch.Tensor, n_ids: Optional[int] = None, return_moments: bool = False):
    """The boxes of xyz (M, 3) float32 (finite coordinates: the caller checked on the host) under ids (M) int32 or int64; an id
    outside [0, n_ids) belongs to no box.  Returns device tensors (count (I) int32, lo, hi, center (I, 3), axes (I, 3, 3),
    extent, eigenvalues (I, 3) float32), the bits of utils/boxes.py's instance_boxes_host.  No read-back with n_ids; with
    n_ids = None one, of max(ids) + 1.  return_moments (tests): the (I, 3) means and (I, 6) covariances, float64, come last."""
    _dev_check(xyz, ids)
    M = xyz.shape[0]
    assert xyz.dtype == F32 and xyz.is_contiguous() and xyz.shape == (M, 3) and 1 <= M < 2 ** 31 - 1
    assert ids.dtype in (torch.int32, torch.int64) and ids.is_contiguous() and ids.shape == (M,)
    dev = xyz.device
    I = max(int(ids.max().item()) + 1, 0) if n_ids is None else int(n_ids)      # (the one read-back)
    assert 0 <= I < 2 ** 31 - 1 and (I >= 1 or n_ids is None)
    count = torch.empty(I, dtype=torch.int32, device=dev)
    lo, hi, center, extent, lam = (torch.empty((I, 3), dtype=F32, device=dev) for _ in range(5))
    axes = torch.empty((I, 3, 3), dtype=F32, device=dev)
    mean = torch.empty((I, 3), dtype=torch.float64, device=dev) if return_moments else None
    cov = torch.empty((I, 6), dtype=torch.float64, device=dev) if return_moments else None
    if I > 0:
        lib = H.lib()
        ws = boxes_workspace(dev, M, I)
        H.check(lib.rl_boxes_sort(ids.data_ptr(), ids.element_size(), M, I, ws.data_ptr(), ws.numel(), _st()), "rl_boxes_sort")
        H.check(lib.rl_boxes_moments(xyz.data_ptr(), M, I, H.ptr(mean), H.ptr(cov), ws.data_ptr(), ws.numel(), _st()),
                "rl_boxes_moments")
        H.check(lib.rl_boxes_fit(xyz.data_ptr(), M, I, count.data_ptr(), lo.data_ptr(), hi.data_ptr(), center.data_ptr(),
                                 axes.data_ptr(), extent.data_ptr(), lam.data_ptr(), ws.data_ptr(), ws.numel(), _st()),
                "rl_boxes_fit")
    res = (count, lo, hi, center, axes, extent, lam)
    return res + (mean, cov) if return_moments else res


# ------------------------------------------------------------------------------------- normals and curvature of a bare cloud
def estimate_normals(xyz: torch.Tensor, k: int, viewpoint=None, chunk: int = 1 << 20, return_cov: bool = False):
    """(normals (M, 3), curvature (M,)) float32 device tensors of xyz (M, 3) float32 (finite coordinates, 3 <= k <= 64,
    k <= M: the caller checked on the host), the bits of utils/normals.py's estimate_normals_host: rl_knn_f32 with the whole
    cloud as support and the queries in chunks of at most `chunk` points - the index and distance buffers stay at
    chunk * k * 12 bytes whatever M is - each followed by one rl_normals launch.  viewpoint: three numbers or None.
    return_cov (tests): the (M, 6) float64 covariances come third.  No read-back."""
    _dev_check(xyz)
    M = xyz.shape[0]
    k, chunk = int(k), int(chunk)
    assert xyz.dtype == F32 and xyz.shape == (M, 3)
    assert 3 <= k <= H.KNN_MAX_K and k <= M < 2 ** 31 - 1 and chunk >= 1
    dev = xyz.device
    lib = H.lib()
    vp = None
    if viewpoint is not None:
        vp = torch.tensor([float(v) for v in viewpoint], dtype=F32).to(dev)
        assert vp.shape == (3,)
    normals = torch.empty((M, 3), dtype=F32, device=dev)
    curvature = torch.empty(M, dtype=F32, device=dev)
    cov = torch.empty((M, 6), dtype=torch.float64, device=dev) if return_cov else None
    chunks = _query_chunks(M, chunk)
    idx = torch.empty((chunks[0][1], k), dtype=torch.int64, device=dev)
    d2 = torch.empty((chunks[0][1], k), dtype=F32, device=dev)
    for first, Q in chunks:
        _knn_chunk(xyz, xyz[first:], Q, k, idx, d2)
        with _rec("normals", (M, Q, k), Q * (8 * k + 12 * k + 16), Q * (18 * k + 400)):
            H.check(lib.rl_normals(xyz.data_ptr(), M, idx.data_ptr(), first, Q, k, H.ptr(vp), normals.data_ptr(),
                                   curvature.data_ptr(), cov[first:].data_ptr() if return_cov else None, _st()),
                    "rl_normals")
    return (normals, curvature, cov) if return_cov else (normals, curvature)


# ------------------------------------------------------------------------------------ statistical outliers of a bare cloud
def outliers_workspace(device, M: int) -> torch.Tensor:
    """Device scratch of rl_outliers_filter (256-byte aligned: torch's allocator aligns to 512)."""
    return _workspace("rl_outliers_workspace_bytes", device, M)


def statistical_outliers(xyz: torch.Tensor, k: int, std_ratio: float, chunk: int = 1 << 20):
    """(keep (M,) bool, slot (M,) int32, kept (M',) int64, mean_distance (M,) float64, stats) of xyz (M, 3) float32 (finite
    coordinates, 1 <= k <= 63, k + 1 <= M, std_ratio finite and >= 0: the caller checked on the host), device tensors but
    stats = (mean, std, threshold) as Python floats: the bits of utils/outliers.py's statistical_outliers_host.  rl_knn_f32
    for k + 1 rows with the whole cloud as support and the queries in chunks of at most `chunk` points - the index and
    distance buffers stay at chunk * (k + 1) * 12 bytes whatever M is - each followed by one rl_outliers_mean_distance
    launch, then rl_outliers_filter.  One read-back: M' and the three statistics together; a threshold that is not finite
    raises ValueError."""
    from .utils import outliers as O
    _dev_check(xyz)
    M = xyz.shape[0]
    k, chunk = int(k), int(chunk)
    assert xyz.dtype == F32 and xyz.is_contiguous() and xyz.shape == (M, 3)
    assert 1 <= k < H.KNN_MAX_K and k + 1 <= M < 2 ** 31 - 1 and chunk >= 1
    dev = xyz.device
    lib = H.lib()
    k1 = k + 1
    mean = torch.empty(M, dtype=torch.float64, device=dev)
    chunks = _query_chunks(M, chunk)
    idx = torch.empty((chunks[0][1], k1), dtype=torch.int64, device=dev)
    d2 = torch.empty((chunks[0][1], k1), dtype=F32, device=dev)
    for first, Q in chunks:
        _knn_chunk(xyz, xyz[first:], Q, k1, idx, d2)
        with _rec("outliers_mean", (M, Q, k), Q * (4 * k1 + 8), Q * 2 * k1):
            H.check(lib.rl_outliers_mean_distance(d2.data_ptr(), M, first, Q, k, mean.data_ptr(), _st()),
                    "rl_outliers_mean_distance")
    keep = torch.empty(M, dtype=torch.uint8, device=dev)
    slot = torch.empty(M, dtype=torch.int32, device=dev)
    kept = torch.empty(M, dtype=torch.int64, device=dev)
    stats = torch.empty(4, dtype=torch.float64, device=dev)
    ws = outliers_workspace(dev, M)
    with _rec("outliers_filter", (M,), M * 45, M * 6):
        H.check(lib.rl_outliers_filter(mean.data_ptr(), M, float(std_ratio), keep.data_ptr(), slot.data_ptr(), kept.data_ptr(),
                                       stats.data_ptr(), ws.data_ptr(), ws.numel(), _st()), "rl_outliers_filter")
    mu, sigma, thr, n_kept = stats.tolist()                        # the read-back
    O.check_threshold(thr)
    return keep.view(torch.bool), slot, kept[:int(n_kept)], mean, (mu, sigma, thr)


# ------------------------------------------------------------------------------------------- RANSAC planes of a bare cloud
def planes_workspace(device, M: int, T: int) -> torch.Tensor:
    """Device scratch of rl_planes_count / rl_planes_split (256-byte aligned: torch's allocator aligns to 512)."""
    return _workspace("rl_planes_workspace_bytes", device, M, T)


def fit_plane(xyz: torch.Tensor, triples, threshold: float, axis=None, cos_min: float = 0.0):
    """The dominant plane of xyz (M, 3) float32 (finite coordinates, M >= 3, threshold a float32 value > 0: the caller checked
    on the host) among the hypotheses of `triples` (T, 3) int64, a numpy array drawn on the host; axis: None or (3,) float32.
    Returns (plane (4,) float32 numpy, inlier (M,) bool, slot (M,) int32, kept (M',) int64, count, best, counts (T,) int32,
    hypotheses (T, 4) float32, centroid (3,) float64 numpy) - device tensors unless marked -, the bits of utils/planes.py's
    fit_plane_host.  rl_planes_hypotheses, rl_planes_count and rl_planes_split under the best hypothesis, the refinement's
    moments by instance_boxes(xyz, inlier - 1, 1, return_moments=True), its float64 step on the host by the twin's own
    refined_plane, and rl_planes_split once more under the refined plane.  Two read-backs: (index flag, best, count, M', the
    best hypothesis, mean, covariance) together, then M' of the refined plane; one when the best count is below 3."""
    from .utils import planes as P
    import numpy as np
    _dev_check(xyz)
    M, T = xyz.shape[0], int(triples.shape[0])
    assert xyz.dtype == F32 and xyz.is_contiguous() and xyz.shape == (M, 3) and 3 <= M < 2 ** 31 - 1
    assert triples.dtype == np.int64 and triples.shape == (T, 3) and 1 <= T <= P.MAX_HYPOTHESES
    dev = xyz.device
    lib = H.lib()
    thr = float(threshold)
    tri = torch.from_numpy(np.ascontiguousarray(triples)).to(dev)
    hyp = torch.empty((T, 4), dtype=F32, device=dev)
    counts = torch.empty(T, dtype=torch.int32, device=dev)
    flags = torch.empty(4, dtype=torch.int32, device=dev)           # [bad index, best, best count, -]
    inlier = torch.empty(M, dtype=torch.uint8, device=dev)
    slot = torch.empty(M, dtype=torch.int32, device=dev)
    kept = torch.empty(M, dtype=torch.int64, device=dev)
    n_kept = torch.empty(1, dtype=torch.int64, device=dev)
    ws = planes_workspace(dev, M, T)
    ax = None if axis is None else (C.c_float * 3)(*(float(a) for a in axis))
    best_ptr = flags[1:].data_ptr()

    def split(plane, best):
        with _rec("planes_split", (M,), M * 45, M * 14):
            H.check(lib.rl_planes_split(xyz.data_ptr(), M, plane.data_ptr(), best, thr, inlier.data_ptr(), slot.data_ptr(),
                                        kept.data_ptr(), n_kept.data_ptr(), ws.data_ptr(), ws.numel(), _st()),
                    "rl_planes_split")

    with _rec("planes_hyp", (M, T), T * 76, T * 40):
        H.check(lib.rl_planes_hypotheses(xyz.data_ptr(), M, tri.data_ptr(), T, ax, float(cos_min), hyp.data_ptr(),
                                         flags.data_ptr(), _st()), "rl_planes_hypotheses")
    with _rec("planes_count", (M, T), 12 * M + 20 * T, 8 * M * T):
        H.check(lib.rl_planes_count(xyz.data_ptr(), M, hyp.data_ptr(), T, thr, counts.data_ptr(), best_ptr, ws.data_ptr(),
                                    ws.numel(), _st()), "rl_planes_count")
    split(hyp, best_ptr)
    mean, cov = instance_boxes(xyz, inlier.to(torch.int32) - 1, 1, return_moments=True)[-2:]
    first = hyp[flags[1].clamp(min=0).long()]
    head = torch.cat((flags[:3].double(), n_kept.double(), first.double(), mean.view(-1), cov.view(-1))).tolist()   # read-back 1
    if head[0] != 0.0:
        raise ValueError(f"fit_plane: triples hold an index outside [0, {M})")
    best, count = int(head[1]), int(head[2])
    centroid = np.full(3, np.nan, np.float64)
    if best < 0:
        plane = np.full(4, np.nan, np.float32)
    elif count < 3:
        plane = np.array(head[4:8], np.float64).astype(np.float32)
    else:
        centroid = np.array(head[8:11], np.float64)
        plane = P.refined_plane(centroid, np.array(head[11:17], np.float64))
        split(torch.from_numpy(plane).to(dev), None)
        head[3] = float(n_kept.item())                                                                            # read-back 2
        count = M - int(head[3])
    return plane, inlier.view(torch.bool), slot, kept[:int(head[3])], count, best, counts, hyp, centroid


def segment_planes(xyz: torch.Tensor, threshold: float, max_planes: int, min_points: int, iterations: int, seed, axis=None,
                   cos_min: float = 0.0):
    """Up to max_planes planes of xyz (M, 3) float32 peeled one after the other (checked arguments: utils/planes.py's
    check_segmentation).  Returns (planes (P, 4) float32 and counts (P,) int64 as numpy arrays, plane_id (M,) int32, kept (M',)
    int64 and slot (M,) int32 as device tensors), the bits of segment_planes_host.  Per round one fit_plane on the cloud that is
    left - its triples drawn on the host from the one generator of `seed` -, which is then index_selected by `kept` and stays
    on the device; at most two read-backs per round."""
    from .utils import planes as P
    import numpy as np
    _dev_check(xyz)
    M = xyz.shape[0]
    dev = xyz.device
    rng = np.random.default_rng(seed)
    alive = torch.arange(M, dtype=torch.int64, device=dev)
    plane_id = torch.full((M,), -1, dtype=torch.int32, device=dev)
    cloud, planes, counts = xyz, [], []
    while len(planes) < max_planes and cloud.shape[0] >= 3:
        plane, inlier, _, kept, count, best, _, _, _ = fit_plane(cloud, P.draw_triples(rng, cloud.shape[0], iterations),
                                                                 threshold, axis, cos_min)
        if best < 0 or count < min_points:
            break
        plane_id[alive] = plane_id[alive].masked_fill(inlier, len(planes))
        planes.append(plane)
        counts.append(count)
        alive, cloud = alive[kept], torch.index_select(cloud, 0, kept)
    slot = torch.full((M,), -1, dtype=torch.int32, device=dev)
    slot[alive] = torch.arange(alive.shape[0], dtype=torch.int32, device=dev)
    return np.array(planes, np.float32).reshape(-1, 4), np.array(counts, np.int64), plane_id, alive, slot


# ------------------------------------------------------------------------------------------------- depth frames to points
def depth_workspace(device, pixels: int) -> torch.Tensor:
    """Device scratch of rl_depth_points (256-byte aligned: torch's allocator aligns to 512)."""
    return _workspace("rl_depth_workspace_bytes", device, pixels)


def _depth_call(depth, state, filtered, camera, stride, filt, z_lo, z_hi, xyz, pixel, count, ws) -> None:
    import ctypes
    Hh, W = depth.shape
    coeffs = None if camera.coeffs is None else (ctypes.c_float * 5)(*[float(c) for c in camera.coeffs])
    alpha, oma, delta = (0.0, 0.0, 0) if filt is None else (float(filt[0]), float(filt[1]), int(filt[2]))
    with _rec("depth_points", (Hh, W, stride), Hh * W * (2 + (4 if state is not None else 0)) + (Hh * W * 16 if xyz is not None else 0),
              Hh * W * 8):
        H.check(H.lib().rl_depth_points(depth.data_ptr(), H.ptr(state), H.ptr(filtered), W, Hh, int(stride), float(camera.fx),
                                        float(camera.fy), float(camera.ppx), float(camera.ppy), float(camera.depth_scale),
                                        None if coeffs is None else ctypes.addressof(coeffs), alpha, oma, delta, float(z_lo),
                                        float(z_hi), H.ptr(xyz), H.ptr(pixel), H.ptr(count), H.ptr(ws),
                                        0 if ws is None else ws.numel(), _st()), "rl_depth_points")


def depth_points(depth: torch.Tensor, camera, z_lo, z_hi, stride: int = 1, state: Optional[torch.Tensor] = None, filt=None,
                 want_filtered: bool = False):
    """(xyz (M, 3) float32, pixel (M,) int32, filtered (H, W) uint16 or None) of depth (H, W) uint16, a contiguous device
    tensor that need only be 2-byte aligned (the caller checked it, the camera - utils/depth.py's DepthCamera -, z_lo < z_hi
    and the stride on the host): the bits of utils/depth.py's deproject_host, after its temporal filter when `state` (H, W)
    uint16 - updated in place - and filt = (alpha, one_minus_alpha, delta) are given.  rl_depth_points: three launches.  One
    read-back, of M; xyz and pixel are the leading rows of buffers of H * W rows."""
    _dev_check(depth, state)
    Hh, W = depth.shape
    assert depth.dtype == torch.uint16 and 1 <= Hh * W < 2 ** 31
    assert (state is None) == (filt is None)
    assert state is None or (state.dtype == torch.uint16 and state.shape == depth.shape)
    dev = depth.device
    P = Hh * W
    xyz = torch.empty((P, 3), dtype=F32, device=dev)
    pixel = torch.empty(P, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    filtered = torch.empty((Hh, W), dtype=torch.uint16, device=dev) if want_filtered else None
    ws = depth_workspace(dev, P)
    _depth_call(depth, state, filtered, camera, stride, filt, z_lo, z_hi, xyz, pixel, count, ws)
    M = int(count.item())                                          # the read-back
    return xyz[:M], pixel[:M], filtered


def temporal_filter(depth: torch.Tensor, state: torch.Tensor, alpha, one_minus_alpha, delta: int) -> torch.Tensor:
    """The filtered frame (H, W) uint16 of depth (H, W) uint16 against state (H, W) uint16, which is updated in place:
    utils/depth.py's temporal_host.  rl_depth_points without outputs for the points: one launch, no read-back."""
    from .utils import depth as D
    _dev_check(depth, state)
    assert depth.dtype == torch.uint16 and state.dtype == torch.uint16 and state.shape == depth.shape and depth.dim() == 2
    filtered = torch.empty(depth.shape, dtype=torch.uint16, device=depth.device)
    camera = D.DepthCamera(depth.shape[1], depth.shape[0], 1.0, 1.0, 0.0, 0.0, 1.0)        # (not read: no point is made)
    _depth_call(depth, state, filtered, camera, 1, (alpha, one_minus_alpha, delta), 0.0, 1.0, None, None, None, None)
    return filtered


# ------------------------------------------------------------------------------------- rigid registration of two clouds (ICP)
ICP_CHUNK = 1024               # FS_CHUNK of csrc/rl_fixedsum.h: the rows of one rl_icp_sums call start and end at chunks


def icp_workspace(device, Ms: int) -> torch.Tensor:
    """Device scratch of rl_icp_sums / rl_icp_fold (256-byte aligned: torch's allocator aligns to 512)."""
    return _workspace("rl_icp_workspace_bytes", device, Ms)


def _icp_rt(T: np.ndarray):
    """The twelve floats of rl_icp_transform from T (4, 4) float64: float32(R) row-major, then float32(t)."""
    R, t = T[:3, :3].astype(np.float32), T[:3, 3].astype(np.float32)
    return (C.c_float * 12)(*[float(v) for v in R.ravel()], *[float(v) for v in t])


def icp_transform(xyz: torch.Tensor, T: np.ndarray, out: Optional[torch.Tensor] = None, first: int = 0, Q: Optional[int] = None
                  ) -> torch.Tensor:
    """xyz (M, 3) float32 moved by T (4, 4) float64, the bits of utils/registration.py's transform_host: rows first ..
    first+Q-1 (all by default) of `out` (a new tensor by default) by one rl_icp_transform launch."""
    _dev_check(xyz, out)
    M = xyz.shape[0]
    assert xyz.dtype == F32 and xyz.is_contiguous() and xyz.shape == (M, 3)
    out = torch.empty_like(xyz) if out is None else out
    Q = M - first if Q is None else Q
    with _rec("icp_transform", (M, Q), 24 * Q, 18 * Q):
        H.check(H.lib().rl_icp_transform(xyz.data_ptr(), M, first, Q, _icp_rt(T), out.data_ptr(), _st()), "rl_icp_transform")
    return out


def icp(source: torch.Tensor, target: torch.Tensor, normals: Optional[torch.Tensor], chk, chunk: int = 1 << 20):
    """utils/registration.py's icp on device tensors: source (Ms, 3), target (Mt, 3) and - for the plane metric - normals
    (Mt, 3), float32 and finite, and chk the checked parameters (the caller checked all of it on the host).  Per evaluation,
    in chunks of at most `chunk` queries (rounded down to a multiple of 1024) so that the index and distance buffers stay at
    chunk * 12 bytes whatever Ms is: rl_icp_transform, rl_knn_f32 (B = 1, k = 1, grid workspace), rl_icp_sums; then
    rl_icp_fold and the one read-back of 30 doubles.  The update is registration.run's, the twin's own code.  Returns (T,
    fitness, inlier_rmse, count, updates, status, correspondence (Ms,) int64 DEVICE, history, transformed (Ms, 3) DEVICE):
    source, target, normals and q never leave HBM."""
    from .utils import registration as R
    _dev_check(source, target, normals)
    Ms, Mt = source.shape[0], target.shape[0]
    metric = int(chk.metric)
    assert source.dtype == F32 and source.is_contiguous() and source.shape == (Ms, 3)
    assert target.dtype == F32 and target.is_contiguous() and target.shape == (Mt, 3)
    assert metric == 1 or (normals is not None and normals.dtype == F32 and normals.is_contiguous() and normals.shape == (Mt, 3))
    assert 1 <= Ms < 2 ** 31 - 1 and 1 <= Mt < 2 ** 31 - 1
    dev = source.device
    lib = H.lib()
    chunks = _query_chunks(Ms, chunk, ICP_CHUNK)
    q = torch.empty((Ms, 3), dtype=F32, device=dev)
    corr = torch.empty(Ms, dtype=torch.int64, device=dev)
    out = torch.empty(R.COLUMNS + 1, dtype=torch.float64, device=dev)
    idx = torch.empty((chunks[0][1], 1), dtype=torch.int64, device=dev)
    d2 = torch.empty((chunks[0][1], 1), dtype=F32, device=dev)
    ws = icp_workspace(dev, Ms)
    knn_ws = {Q: _knn_workspace(dev, 1, Mt, Q, 1, False) for Q in {Q for _, Q in chunks}}
    gate2 = float(chk.g2)
    flops = 100 if metric == 0 else 300

    def evaluate(T):
        for first, Q in chunks:
            icp_transform(source, T, q, first, Q)
            _knn_chunk(target, q[first:], Q, 1, idx, d2, knn_ws[Q])
            with _rec("icp_sums", (Ms, Mt, Q, metric), Q * (32 + (24 if metric == 0 else 12)), Q * flops):
                H.check(lib.rl_icp_sums(q.data_ptr(), H.ptr(normals), target.data_ptr(), Mt, idx.data_ptr(), d2.data_ptr(), Ms,
                                        first, Q, gate2, metric, corr.data_ptr(), ws.data_ptr(), ws.numel(), _st()),
                        "rl_icp_sums")
        with _rec("icp_fold", (Ms,), ws.numel(), 0):
            H.check(lib.rl_icp_fold(Ms, out.data_ptr(), ws.data_ptr(), ws.numel(), _st()), "rl_icp_fold")
        return out.cpu().numpy()                                       # the read-back

    res = R.run(evaluate, Ms, chk)
    return res[:6] + (corr, res[6], q)


# --------------------------------------------------------------------------- FPFH descriptors, matching, global registration
def fpfh(xyz: torch.Tensor, normals: torch.Tensor, k: int, chunk: int = 1 << 20):
    """(descriptor (M, 33) float32, code (M, 36) uint8, spfh (M, 33) uint8) device tensors of xyz and normals (M, 3) float32
    (finite, 2 <= k <= 63, k + 1 <= M: the caller checked on the host), the bits of utils/features.py's fpfh_host: rl_knn_f32
    for k + 1 rows with the whole cloud as support and the queries in chunks of at most `chunk` points, each followed by one
    rl_fpfh_spfh launch; then rl_fpfh_fpfh per chunk, which reads the neighbours' finished SPFH rows - so the index and
    distance rows of the WHOLE cloud are kept, M * (k + 1) * 12 bytes.  No read-back."""
    _dev_check(xyz, normals)
    M = xyz.shape[0]
    k, chunk = int(k), int(chunk)
    assert xyz.dtype == F32 and xyz.shape == (M, 3) and normals.dtype == F32 and normals.shape == (M, 3)
    assert 2 <= k < H.KNN_MAX_K and k + 1 <= M < 2 ** 31 - 1 and chunk >= 1
    dev = xyz.device
    lib = H.lib()
    k1 = k + 1
    idx = torch.empty((M, k1), dtype=torch.int64, device=dev)
    d2 = torch.empty((M, k1), dtype=F32, device=dev)
    spfh = torch.empty((M, 33), dtype=torch.uint8, device=dev)
    desc = torch.empty((M, 33), dtype=F32, device=dev)
    code = torch.empty((M, 36), dtype=torch.uint8, device=dev)
    chunks = _query_chunks(M, chunk)
    for first, Q in chunks:
        _knn_chunk(xyz, xyz[first:], Q, k1, idx[first:], d2[first:])
        with _rec("fpfh_spfh", (M, Q, k), Q * (12 * k1 + 24 * k1 + 33), Q * k * 90):
            H.check(lib.rl_fpfh_spfh(xyz.data_ptr(), normals.data_ptr(), M, idx[first:].data_ptr(), d2[first:].data_ptr(), first,
                                     Q, k, spfh.data_ptr(), _st()), "rl_fpfh_spfh")
    for first, Q in chunks:
        with _rec("fpfh_fpfh", (M, Q, k), Q * (12 * k1 + 33 * k + 168), Q * k * 66):
            H.check(lib.rl_fpfh_fpfh(spfh.data_ptr(), M, idx[first:].data_ptr(), d2[first:].data_ptr(), first, Q, k,
                                     desc.data_ptr(), code.data_ptr(), _st()), "rl_fpfh_fpfh")
    return desc, code, spfh


def match_features(code_source: torch.Tensor, code_target: torch.Tensor):
    """(idx (Ms,) int64, dist (Ms,) int32) device tensors: for every row of code_source (Ms, 36) uint8 the nearest row of
    code_target (Mt, 36) uint8, the bits of utils/features.py's match_features_host.  rl_match_u8: three launches, no
    read-back."""
    _dev_check(code_source, code_target)
    Ms, Mt = code_source.shape[0], code_target.shape[0]
    assert code_source.dtype == torch.uint8 and code_source.shape == (Ms, 36) and 1 <= Ms < 2 ** 31 - 1
    assert code_target.dtype == torch.uint8 and code_target.shape == (Mt, 36) and 1 <= Mt < 2 ** 31 - 1
    dev = code_source.device
    idx = torch.empty(Ms, dtype=torch.int64, device=dev)
    dist = torch.empty(Ms, dtype=torch.int32, device=dev)
    ws = _workspace("rl_match_workspace_bytes", dev, Ms, Mt)
    with _rec("match_u8", (Ms, Mt), 36 * (Ms + Mt) + 12 * Ms, 2 * 36 * Ms * Mt):
        H.check(H.lib().rl_match_u8(code_source.data_ptr(), Ms, code_target.data_ptr(), Mt, idx.data_ptr(), dist.data_ptr(),
                                    ws.data_ptr(), ws.numel(), _st()), "rl_match_u8")
    return idx, dist


def global_workspace(device, C: int, T: int) -> torch.Tensor:
    """Device scratch of rl_global_hypotheses / rl_global_count / rl_global_sums (256-byte aligned)."""
    return _workspace("rl_global_workspace_bytes", device, C, T)


def global_ransac(source: torch.Tensor, target: torch.Tensor, corr: torch.Tensor, triples, s2: float, gate2: float):
    """The RANSAC of utils/registration.py's global_registration on device tensors: source (C, 3) and target (Mt, 3) float32,
    corr (C,) int64 in [0, Mt), triples (T, 3) int64, a numpy array drawn on the host (the caller checked all of it).
    rl_global_hypotheses and rl_global_count, one read-back of (flag, counts); the hypotheses come back once; then
    registration.global_run, the twin's own decisions, around rl_global_sums - one read-back of sixteen doubles per call, at
    most two calls.  Returns (T (4, 4) float64, count, inlier (C,) bool DEVICE or None, best, counts (T,) int32 numpy,
    hypotheses (T, 12) float32 numpy, sums (16,) float64, status)."""
    from .utils import registration as R
    _dev_check(source, target, corr)
    C, Mt, T = source.shape[0], target.shape[0], int(triples.shape[0])
    assert source.dtype == F32 and source.shape == (C, 3) and target.dtype == F32 and target.shape == (Mt, 3)
    assert corr.dtype == torch.int64 and corr.shape == (C,) and 3 <= C < 2 ** 31 - 1 and 1 <= Mt < 2 ** 31 - 1
    assert triples.dtype == np.int64 and triples.shape == (T, 3) and 1 <= T <= R.MAX_HYPOTHESES
    dev = source.device
    lib = H.lib()
    tri = torch.from_numpy(np.ascontiguousarray(triples)).to(dev)
    hyp = torch.empty((T, 12), dtype=F32, device=dev)
    head = torch.empty(T + 1, dtype=torch.int32, device=dev)          # [bad index, counts]
    inlier = torch.empty(C, dtype=torch.uint8, device=dev)
    out = torch.empty(R.SUM_COLUMNS, dtype=torch.float64, device=dev)
    ws = global_workspace(dev, C, T)

    def hyp_counts():
        with _rec("global_hyp", (C, T), T * 192, T * 150):
            H.check(lib.rl_global_hypotheses(source.data_ptr(), C, target.data_ptr(), Mt, corr.data_ptr(), tri.data_ptr(), T,
                                             float(s2), hyp.data_ptr(), head.data_ptr(), ws.data_ptr(), ws.numel(), _st()),
                    "rl_global_hypotheses")
        with _rec("global_count", (C, T), 48 * C + 52 * T, 31 * C * T):
            H.check(lib.rl_global_count(source.data_ptr(), C, target.data_ptr(), Mt, corr.data_ptr(), hyp.data_ptr(), T,
                                        float(gate2), head[1:].data_ptr(), ws.data_ptr(), ws.numel(), _st()), "rl_global_count")
        got = head.cpu().numpy()                                       # the read-back
        if got[0] != 0:
            raise ValueError(f"global_registration: triples or correspondences hold an index outside [0, {C}) / [0, {Mt})")
        return hyp.cpu().numpy(), got[1:].copy()

    def sums_of(M):
        with _rec("global_sums", (C,), 44 * C, 60 * C):
            H.check(lib.rl_global_sums(source.data_ptr(), C, target.data_ptr(), Mt, corr.data_ptr(), _icp_rt(M), float(gate2),
                                       inlier.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), _st()), "rl_global_sums")
        return out.cpu().numpy(), inlier.view(torch.bool)              # the read-back

    return R.global_run(hyp_counts, sums_of, C)


# ------------------------------------------------------------------------------------------- TSDF fusion of depth frames
def tsdf_workspace(device, voxels: int) -> torch.Tensor:
    """Device scratch of rl_tsdf_count / rl_tsdf_points (256-byte aligned: torch's allocator aligns to 512)."""
    return _workspace("rl_tsdf_workspace_bytes", device, voxels)


def _tsdf_volume(tsdf: torch.Tensor, weight: torch.Tensor, origin, voxel):
    """The leading arguments every rl_tsdf_* entry shares, from the state (nz, ny, nx) float32 of utils/tsdf.py's TsdfVolume."""
    nz, ny, nx = tsdf.shape
    assert tsdf.dtype == F32 and weight.dtype == F32 and weight.shape == tsdf.shape and 1 <= nx * ny * nz < 2 ** 31
    return tsdf.data_ptr(), weight.data_ptr(), nx, ny, nz, (C.c_float * 3)(*[float(o) for o in origin]), float(voxel)


def tsdf_integrate(tsdf: torch.Tensor, weight: torch.Tensor, origin, voxel, trunc, max_weight: int, depth: torch.Tensor,
                   camera, z_lo, z_hi, w2c: np.ndarray) -> None:
    """One frame - depth (H, W) uint16, a contiguous device tensor that need only be 2-byte aligned - into tsdf and weight
    (nz, ny, nx) float32, in place: the bits of utils/tsdf.py's integrate_host (the caller checked the frame, the camera - a
    DepthCamera without coeffs -, z_lo < z_hi and the pose on the host).  w2c: the twelve float32 of world_to_camera.
    rl_tsdf_integrate: one launch, no read-back."""
    _dev_check(tsdf, weight, depth)
    Hh, W = depth.shape
    assert depth.dtype == torch.uint16 and camera.coeffs is None and w2c.shape == (12,)
    V = tsdf.numel()
    with _rec("tsdf_integrate", (tuple(tsdf.shape), Hh, W), 16 * V + 2 * Hh * W, 60 * V):
        H.check(H.lib().rl_tsdf_integrate(*_tsdf_volume(tsdf, weight, origin, voxel), float(trunc), int(max_weight),
                                          depth.data_ptr(), W, Hh, float(camera.fx), float(camera.fy), float(camera.ppx),
                                          float(camera.ppy), float(camera.depth_scale), float(z_lo), float(z_hi),
                                          (C.c_float * 12)(*[float(v) for v in w2c]), _st()), "rl_tsdf_integrate")


def tsdf_extract(tsdf: torch.Tensor, weight: torch.Tensor, origin, voxel, min_weight: int):
    """(xyz (M, 3) float32, edge (M,) int64) device tensors: the surface points of tsdf and weight (nz, ny, nx) float32, the
    bits of utils/tsdf.py's extract_host.  rl_tsdf_count (two launches), one read-back, of M, outputs of exactly M rows,
    rl_tsdf_points (one launch; none for M = 0)."""
    _dev_check(tsdf, weight)
    dev = tsdf.device
    V = tsdf.numel()
    lib = H.lib()
    count = torch.empty(1, dtype=torch.int64, device=dev)
    ws = tsdf_workspace(dev, V)
    with _rec("tsdf_count", tuple(tsdf.shape), 8 * V, 12 * V):
        H.check(lib.rl_tsdf_count(*_tsdf_volume(tsdf, weight, origin, voxel), int(min_weight), count.data_ptr(), ws.data_ptr(),
                                  ws.numel(), _st()), "rl_tsdf_count")
    M = int(count.item())                                          # the read-back
    if not 0 <= M < 2 ** 32:
        raise H.HipKernelError(f"rl_tsdf_count: {M} surface points, outside 0 .. 2^32 - 1")
    xyz = torch.empty((M, 3), dtype=F32, device=dev)
    edge = torch.empty(M, dtype=torch.int64, device=dev)
    if M:
        with _rec("tsdf_points", tuple(tsdf.shape), 8 * V + 20 * M, 12 * V):
            H.check(lib.rl_tsdf_points(*_tsdf_volume(tsdf, weight, origin, voxel), int(min_weight), M, xyz.data_ptr(),
                                       edge.data_ptr(), xyz.shape[0], ws.data_ptr(), ws.numel(), _st()), "rl_tsdf_points")
    return xyz, edge
