"""Launch plan of the concat-gather A operand of rl_gemm (rl_gemm_desc.a2_*), without a GPU.

plan_gemm alone decides support: where the LDS-DMA wide kernel takes the product of the stored concatenation in one pass (bf16x3 /
bf16 arithmetic with pre-split weights, "dma" staging, no K split), fp32 rows, K == 2 * a2_split <= 1024, a2_split % 32 == 0 and
rows per cloud a multiple of 16 (hence M % 16 == 0).  rl_gemm_concat_supported answers with the return code of rl_gemm's own
validation and plan and launches nothing; the descriptors carry 16-byte-aligned dummy addresses that are compared, never
dereferenced.
"""
import ctypes as C

import pytest

_A, _A2, _IDX, _W, _WS, _Y, _SC, _SH = (0x10000000 + 0x100000 * i for i in range(8))
OK, ERR_ARGS, ERR_UNSUPPORTED = 0, -1, -4

SHAPES = [(576, 128, 128), (1728, 128, 128), (1728, 256, 256), (20480, 256, 256), (81920, 256, 256), (4096, 512, 512),
          (1024, 1024, 256), (2048, 64, 128)]


def _desc(H, M, N, K, split=0, B=1, fold2=True, W_split=_WS):
    d = H.GemmDesc()
    d.A, d.lda, d.a_bstride, d.a_mode = _A, (split or K), M // B, 0
    d.B, d.n, d.N, d.K = B, M // B, N, K
    d.W, d.w_ks, d.w_ns, d.W_split = _W, 1, K, W_split
    d.Y, d.ldy, d.y_bstride = _Y, N, M // B
    if split:
        d.a2_split, d.A2, d.lda2, d.a2_bstride, d.a2_idx = split, _A2, K - split, 4096, _IDX
        if fold2:
            d.a2_scale, d.a2_shift, d.a2_act, d.a2_slope = _SC, _SH, H.ACT_LRELU, 0.2
    return d


@pytest.fixture()
def lib():
    from randlanet import _hip as H
    L = H.lib()
    mode0 = L.rl_get_wide_gemm()
    yield H, L
    L.rl_set_wide_gemm(mode0)
    L.rl_set_wgemm_staging(b"dma")
    L.rl_set_wgemm_tile(b"auto")


def _ordinary_answers(H, L):
    out = []
    for M, K, N in SHAPES:
        out.append((int(L.rl_gemm_stat_slots(M, N, K)), int(L.rl_gemm_kslab_floats(M, N, K)),
                    int(L.rl_gemm_streams(C.byref(_desc(H, M, N, K)))), int(L.rl_gemm_concat_supported(C.byref(_desc(H, M, N, K))))))
    return out


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("tile", ["auto", "64x128", "64x64"])
def test_supported_on_every_tile_shape_and_launches_nothing(lib, mode, tile):
    H, L = lib
    assert L.rl_set_wide_gemm(mode.encode()) == 0 and L.rl_set_wgemm_tile(tile.encode()) == 0
    before = _ordinary_answers(H, L)
    launches = L.rl_launch_count()
    for M, K, N in SHAPES:
        for B in (1, 2) if M % 32 == 0 else (1, 3):
            for fold2 in (True, False):
                d = _desc(H, M, N, K, K // 2, B=B, fold2=fold2)
                assert L.rl_gemm_concat_supported(C.byref(d)) == OK, (M, K, N, B, L.rl_last_error())
    assert L.rl_launch_count() == launches
    # the queries about ordinary operands answer what they answered before the concat operands were planned
    assert _ordinary_answers(H, L) == before
    assert all(a[3] == OK for a in before)


def test_stat_slots_do_not_depend_on_the_operand(lib):
    H, L = lib
    assert L.rl_set_wide_gemm(b"bf16x3") == 0
    # (the slot count is a function of the shape alone: the same call answers for both operands)
    assert int(L.rl_gemm_stat_slots(1728, 256, 256)) == 27 and int(L.rl_gemm_stat_slots(81920, 256, 256)) == 640
    assert int(L.rl_gemm_stat_slots(20480, 256, 256)) == 160


UNSUPPORTED = {
    # name: (mode, staging, tile, M, B, N, K, split, W_split)
    "split 48": ("bf16x3", "dma", "auto", 1728, 1, 128, 96, 48, _WS),
    "split 16": ("bf16x3", "dma", "auto", 1728, 1, 128, 32, 16, _WS),
    "K = 3 * split": ("bf16x3", "dma", "auto", 1728, 1, 128, 192, 64, _WS),
    "K = 4 * split": ("bf16", "dma", "auto", 1728, 1, 128, 256, 64, _WS),
    "K = 2048": ("bf16x3", "dma", "auto", 1728, 1, 128, 2048, 1024, _WS),
    "fp32 arithmetic": ("fp32", "dma", "auto", 1728, 1, 256, 256, 128, _WS),
    "no pre-split weight": ("bf16x3", "dma", "auto", 1728, 1, 256, 256, 128, None),
    "register staging": ("bf16x3", "registers", "auto", 1728, 1, 256, 256, 128, _WS),
    "M % 16 = 8": ("bf16x3", "dma", "auto", 1736, 1, 256, 256, 128, _WS),
    "rows per cloud % 16 = 8": ("bf16x3", "dma", "auto", 1744, 2, 256, 256, 128, _WS),
    "a K split (one tile shape with few tiles)": ("bf16x3", "dma", "128", 1728, 1, 256, 256, 128, _WS),
    "the streaming kernel's shapes": ("bf16x3", "dma", "128", 20480, 1, 64, 64, 32, _WS),
}


@pytest.mark.parametrize("name", sorted(UNSUPPORTED))
def test_everything_else_is_unsupported_and_launches_nothing(lib, name):
    H, L = lib
    mode, staging, tile, M, B, N, K, split, ws = UNSUPPORTED[name]
    assert L.rl_set_wide_gemm(mode.encode()) == 0 and L.rl_set_wgemm_staging(staging.encode()) == 0
    assert L.rl_set_wgemm_tile(tile.encode()) == 0
    launches = L.rl_launch_count()
    d = _desc(H, M, N, K, split, B=B, W_split=ws)
    rc = L.rl_gemm_concat_supported(C.byref(d))
    assert rc == ERR_UNSUPPORTED, (name, rc, L.rl_last_error())
    assert L.rl_last_error().startswith(b"rl_gemm:")
    # rl_gemm itself refuses with the same code before it launches anything
    assert L.rl_gemm(C.byref(d), None) == ERR_UNSUPPORTED
    assert L.rl_launch_count() == launches
    # ... and the stored operand of the same shape is planned as ever
    assert L.rl_gemm_concat_supported(C.byref(_desc(H, M, N, K, W_split=ws))) == OK


def test_bf16_rows_are_not_an_operand_of_rl_gemm():
    """rl_gemm reads the rows of a concat-gather operand as fp32 and rl_gemm_desc has no storage flag for them, so this one rule
    is not the plan's: ops.gemm_concat_supported answers it from the tensors' dtype before it fills a descriptor or asks the
    library (no device is needed for the answer; with fp32 rows the same call goes on to the library and needs one - the GPU
    file has that half).  Either source in bf16 is a refusal, and so it is for the attentive pooling's query."""
    import torch

    from randlanet import _ops as ops
    W = torch.zeros((256, 256), dtype=torch.float32)
    idx = torch.zeros((1, 2, 16), dtype=torch.int32)
    for du, dg in ((torch.bfloat16, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)):
        u = ops.Lazy(torch.zeros((32, 128), dtype=du), 1, 32, 32, 128)
        g = ops.Lazy(torch.zeros((2, 128), dtype=dg), 1, 2, 2, 128)
        x = ops.ConcatGather(u, g, idx)
        assert ops.gemm_concat_supported(x, W, 1, 256, 256, None) is False, (du, dg)
        assert ops.attpool_concat_supported(x, 2, 16) is False, (du, dg)


def test_incomplete_second_source_is_an_argument_error(lib):
    H, L = lib
    assert L.rl_set_wide_gemm(b"bf16x3") == 0
    for edit in (dict(A2=None), dict(a2_idx=None), dict(a2_bstride=0), dict(a2_shift=None), dict(A2=_A2 + 4), dict(lda2=126),
                 dict(lda2=124), dict(a2_split=256), dict(a2_split=-32), dict(a_mode=1), dict(a2_idx=_IDX + 2)):
        d = _desc(H, 1728, 256, 256, 128)
        for k, v in edit.items():
            setattr(d, k, v)
        assert L.rl_gemm_concat_supported(C.byref(d)) == ERR_ARGS, edit


def test_setter_round_trip():
    from randlanet import _hip as H
    L = H.lib()
    mode0 = L.rl_get_pool256_x()
    try:
        assert mode0 in (b"in_place", b"stored")
        for m in (b"stored", b"in_place"):
            assert L.rl_set_pool256_x(m) == 0 and L.rl_get_pool256_x() == m
        assert L.rl_set_pool256_x(b"sometimes") == ERR_ARGS and L.rl_set_pool256_x(None) == ERR_ARGS
        assert L.rl_get_pool256_x() == b"in_place"
    finally:
        L.rl_set_pool256_x(mode0)
