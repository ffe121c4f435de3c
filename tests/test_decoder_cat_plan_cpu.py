"""Launch plans of the decoder's concat operand ([gathered | direct], a2_first = 1) and of the streaming split store, without a GPU.

plan_gemm / plan_wgrad alone decide: rl_gemm_concat_supported and rl_wgrad_plan answer with the return code of the entry points'
own validation and plan and launch nothing.  The descriptors carry 16-byte-aligned dummy addresses that are compared, never
dereferenced.  The shapes are those tests/test_decoder_cat_gpu.py runs.
"""
import ctypes as C
import os

import pytest

_A, _A2, _IDX, _W, _WS, _Y, _SC, _SH, _DY, _SLAB, _O2 = (0x10000000 + 0x100000 * i for i in range(11))
OK, ERR_ARGS, ERR_UNSUPPORTED = 0, -1, -4

# B, rows per cloud, C1 = C2, N
WIDE = [(2, 48, 128, 32), (3, 80, 256, 128), (2, 16, 512, 256)]
STREAM = [(2, 48, 32, 8), (3, 1000, 32, 8), (2, 48, 16, 8), (2, 48, 32, 16)]


def _gemm(H, B, n, h, N, first=1, cat=True, ws=_WS):
    d = H.GemmDesc()
    K = 2 * h
    d.A, d.lda, d.a_bstride, d.a_mode = _A, (h if cat else K), n, 0
    d.B, d.n, d.N, d.K = B, n, N, K
    d.W, d.w_ks, d.w_ns, d.W_split = _W, 1, K, ws
    d.Y, d.ldy, d.y_bstride = _Y, N, n
    if cat:
        d.a2_split, d.A2, d.lda2, d.a2_bstride, d.a2_idx, d.a2_first = h, _A2, h + 8, n // 4 + 3, _IDX, first
        d.a2_scale, d.a2_shift, d.a2_act = _SC, _SH, H.ACT_RELU
    return d


def _wgrad(H, B, n, h, N, first=1, cat=True, rows_bf16=0):
    d = H.WgradDesc()
    K = 2 * h
    d.A, d.lda, d.a_bstride, d.a_mode = _A, (h if cat else K), n, 0
    d.B, d.n, d.N, d.K = B, n, N, K
    d.dY, d.lddy, d.dy_bstride = _DY, N, n
    d.dW, d.w_ks, d.w_ns = _W, 1, K
    d.slab, d.slab_floats, d.defer_reduce, d.rows_bf16 = _SLAB, 1 << 62, 1, rows_bf16
    if cat:
        d.a2_split, d.A2, d.lda2, d.a2_bstride, d.a2_idx, d.a2_first = h, _A2, h + 8, n // 4 + 3, _IDX, first
        d.a2_scale, d.a2_shift, d.a2_act = _SC, _SH, H.ACT_RELU
    return d


def _plan(L, d):
    grid, threads, name = (C.c_int32 * 3)(), C.c_int32(0), C.c_char_p()
    rc = L.rl_wgrad_plan(C.byref(d), grid, C.byref(threads), C.byref(name))
    return rc, (tuple(grid), threads.value, name.value) if rc == OK else None


@pytest.fixture()
def lib():
    from randlanet import _hip as H
    L = H.lib()
    mode0 = L.rl_get_wide_gemm()
    yield H, L
    L.rl_set_wide_gemm(mode0)
    L.rl_set_wgemm_staging(b"dma")


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_products_the_plan_takes(lib, mode):
    H, L = lib
    assert L.rl_set_wide_gemm(mode.encode()) == 0
    launches = L.rl_launch_count()
    for B, n, h, N in WIDE + STREAM:
        for first in (1, 0):
            d = _gemm(H, B, n, h, N, first)
            assert L.rl_gemm_concat_supported(C.byref(d)) == OK, (B, n, h, N, first, L.rl_last_error())
        # the stored operand of the same shape is planned as ever
        assert L.rl_gemm_concat_supported(C.byref(_gemm(H, B, n, h, N, cat=False))) == OK
    assert L.rl_launch_count() == launches


GEMM_REFUSED = {
    # name: (mode, staging, B, n, h, N, edits)
    "wide, fp32 arithmetic": ("fp32", "dma", 2, 48, 128, 32, {}),
    "wide, register staging": ("bf16x3", "registers", 3, 80, 256, 128, {}),
    "wide, no pre-split weight": ("bf16x3", "dma", 3, 80, 256, 128, dict(W_split=None)),
    "wide, rows per cloud % 16 = 8": ("bf16x3", "dma", 2, 40, 128, 32, {}),
    "streaming, more than one column block": ("bf16x3", "dma", 2, 48, 32, 64, {}),
    "streaming, split 24": ("bf16x3", "dma", 2, 48, 24, 8, {}),
    "streaming, BatchNorm-backward sums": ("bf16x3", "dma", 2, 48, 32, 8, dict(bnb_Y=_Y, stats=_O2, bnb_scale=_SC, bnb_shift=_SH,
                                                                                bnb_mean=_SC, bnb_invstd=_SH)),
    "streaming, rows that rule out 16-byte loads": ("bf16x3", "dma", 2, 48, 32, 8, dict(A=_A + 4)),
}


@pytest.mark.parametrize("name", sorted(GEMM_REFUSED))
def test_products_the_plan_refuses(lib, name):
    H, L = lib
    mode, staging, B, n, h, N, edits = GEMM_REFUSED[name]
    assert L.rl_set_wide_gemm(mode.encode()) == 0 and L.rl_set_wgemm_staging(staging.encode()) == 0
    d = _gemm(H, B, n, h, N)
    for k, v in edits.items():
        setattr(d, k, v)
    launches = L.rl_launch_count()
    rc = L.rl_gemm_concat_supported(C.byref(d))
    assert rc == ERR_UNSUPPORTED, (name, rc, L.rl_last_error())
    assert L.rl_last_error().startswith(b"rl_gemm:")
    assert L.rl_gemm(C.byref(d), None) == ERR_UNSUPPORTED
    assert L.rl_launch_count() == launches


def test_second_source_sizes_follow_the_column_order(lib):
    """[gathered | direct]: the table holds a2_split columns, the direct rows K - a2_split."""
    H, L = lib
    assert L.rl_set_wide_gemm(b"bf16x3") == 0
    d = _gemm(H, 2, 48, 128, 32)
    d.lda2 = 124
    assert L.rl_gemm_concat_supported(C.byref(d)) == ERR_ARGS
    d = _gemm(H, 2, 48, 128, 32)
    d.lda = 124
    assert L.rl_gemm_concat_supported(C.byref(d)) == ERR_ARGS
    w = _wgrad(H, 2, 48, 128, 32)
    w.lda2 = 124
    assert _plan(L, w)[0] == ERR_ARGS


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_weight_gradients_the_plan_takes(lib, mode):
    H, L = lib
    assert L.rl_set_wide_gemm(mode.encode()) == 0
    launches = L.rl_launch_count()
    for B, n, h, N in WIDE:
        rc0, plain = _plan(L, _wgrad(H, B, n, h, N, cat=False))
        assert rc0 == OK and plain[2] == b"pwgrad128w_kernel"
        for first in (1, 0):
            d = _wgrad(H, B, n, h, N, first)
            assert _plan(L, d) == (OK, plain), (B, n, h, N, first, L.rl_last_error())
            assert L.rl_wgrad_batchable(C.byref(d)) == 1
    for B, n, h, N in STREAM:
        rc0, plain = _plan(L, _wgrad(H, B, n, h, N, cat=False))
        assert rc0 == OK and plain[2] == b"swgrad_kernel"
        for first in (1, 0):
            d = _wgrad(H, B, n, h, N, first)
            rc, got = _plan(L, d)
            assert rc == OK, L.rl_last_error()
            # the ordinary layer's grid and slabs, the concat-gather instantiation
            assert got[:2] == plain[:2] and got[2] == b"swgrad_kernel<cat>"
            assert L.rl_wgrad_batchable(C.byref(d)) == 2
    assert L.rl_launch_count() == launches


def test_weight_gradients_the_plan_refuses(lib):
    H, L = lib
    launches = L.rl_launch_count()
    for mode, B, n, h, N, bf16 in (("fp32", 2, 48, 128, 32, 0), ("bf16x3", 2, 48, 128, 32, 1), ("bf16x3", 2, 48, 32, 8, 1),
                                   ("bf16x3", 2, 48, 32, 32, 0), ("bf16x3", 2, 48, 24, 8, 0)):
        assert L.rl_set_wide_gemm(mode.encode()) == 0
        d = _wgrad(H, B, n, h, N, rows_bf16=bf16)
        rc, _ = _plan(L, d)
        assert rc == ERR_UNSUPPORTED, (mode, B, n, h, N, bf16, rc, L.rl_last_error())
        assert L.rl_last_error().startswith(b"rl_wgrad:")
        assert L.rl_wgrad_batchable(C.byref(d)) == 0
    assert L.rl_launch_count() == launches


def _split(H, M, K, N, split_col, **edits):
    d = H.GemmDesc()
    d.A, d.lda, d.a_bstride, d.a_mode = _A, K, M, 0
    d.B, d.n, d.N, d.K = 1, M, N, K
    d.W, d.w_ks, d.w_ns = _W, N, 1
    d.Y, d.ldy, d.y_bstride = _Y, split_col, M
    d.out2, d.split_col = _O2, split_col
    for k, v in edits.items():
        setattr(d, k, v)
    return d


def test_streaming_split_store_plan(lib):
    H, L = lib
    launches = L.rl_launch_count()
    for M in (40, 4096, 327680):
        for K, N, sc in ((8, 64, 32), (8, 64, 16), (8, 64, 48), (32, 32, 16), (64, 48, 32)):
            assert L.rl_gemm_concat_supported(C.byref(_split(H, M, K, N, sc))) == OK, (M, K, N, sc, L.rl_last_error())
            assert L.rl_gemm_concat_supported(C.byref(_split(H, M, K, N, sc, accumulate=1))) == OK
    refused = [_split(H, 4096, 8, 64, 24), _split(H, 4096, 8, 64, 32, addend=_SC), _split(H, 4096, 8, 64, 32, A=_A + 4),
               _split(H, 4096, 6, 64, 32, lda=6)]
    for d in refused:
        assert L.rl_gemm_concat_supported(C.byref(d)) == ERR_UNSUPPORTED, L.rl_last_error()
        assert b"split-scatter" in L.rl_last_error()
        assert L.rl_gemm(C.byref(d), None) == ERR_UNSUPPORTED
    # statistics have no place in a split epilogue, on any kernel
    assert L.rl_gemm_concat_supported(C.byref(_split(H, 4096, 8, 64, 32, stats=_SLAB))) == ERR_UNSUPPORTED
    assert L.rl_launch_count() == launches


def test_bf16_rows_are_refused_before_the_library_is_asked():
    import torch

    from randlanet import _ops as ops
    W = torch.zeros((8, 64), dtype=torch.float32)
    nn = torch.zeros((1, 32, 1), dtype=torch.int32)
    for dx, ds in ((torch.bfloat16, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)):
        x = ops.Lazy(torch.zeros((8, 32), dtype=dx), 1, 8, 8, 32)
        skip = ops.Lazy(torch.zeros((32, 32), dtype=ds), 1, 32, 32, 32)
        assert ops.gemm_concat_supported(ops.InterpConcat(x, skip, nn), W, 1, 64, 8, None) is False, (dx, ds)
    g = ops.Lazy(torch.zeros((32, 8), dtype=torch.bfloat16), 1, 32, 32, 8)
    assert ops.gemm_split_supported(g, W, 64, 1, 64, 32, None) is False


def test_grouped_launch_table_still_fits_the_kernel_arguments():
    """Eight second sources per grouped launch; the table's size is asserted where it is declared (the library was built)."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3d_recognizer_amd", "csrc", "gemm.hip")
    with open(src) as f:
        text = f.read()
    assert "constexpr int WB_CAT_MAX = 8;" in text
    assert "static_assert(sizeof(WgradBatch) <= 4096" in text


def test_setter_round_trip():
    from randlanet import _hip as H
    L = H.lib()
    mode0 = L.rl_get_decoder_cat()
    try:
        assert mode0 in (b"in_place", b"stored")
        for m in (b"stored", b"in_place"):
            assert L.rl_set_decoder_cat(m) == 0 and L.rl_get_decoder_cat() == m
        assert L.rl_set_decoder_cat(b"sometimes") == ERR_ARGS and L.rl_set_decoder_cat(None) == ERR_ARGS
        assert L.rl_get_decoder_cat() == b"in_place"
    finally:
        L.rl_set_decoder_cat(mode0)
