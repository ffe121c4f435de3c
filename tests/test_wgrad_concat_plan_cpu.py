"""Launch plan of the concat-gather A operand of rl_wgrad (rl_wgrad_desc.a2_*), without a GPU.

plan_wgrad alone decides support: the wide (128 x 128 tile) kernel in the bf16x3 / bf16 arithmetic modes, fp32 rows,
K == 2 * a2_split, a2_split % 16 == 0.  rl_wgrad_plan answers with the return code of rl_wgrad's own validation and plan and
launches nothing; the descriptors carry 16-byte-aligned dummy addresses that are compared, never dereferenced.
"""
import ctypes as C

import pytest

_A, _A2, _IDX, _DY, _DW, _SLAB, _SC, _SH = (0x10000000 + 0x100000 * i for i in range(8))
OK, ERR_ARGS, ERR_UNSUPPORTED = 0, -1, -4


def _desc(H, M, N, K, split=0, rows_bf16=0, fold2=True):
    d = H.WgradDesc()
    d.A, d.lda, d.a_bstride, d.a_mode = _A, (split or K), M, 0
    d.B, d.n, d.N, d.K = 1, M, N, K
    d.dY, d.lddy, d.dy_bstride = _DY, N, M
    d.dW, d.w_ks, d.w_ns = _DW, 1, K
    d.slab, d.slab_floats, d.defer_reduce = _SLAB, 1 << 62, 1
    d.rows_bf16 = rows_bf16
    if split:
        d.a2_split, d.A2, d.lda2, d.a2_bstride, d.a2_idx = split, _A2, (K - split + 3) // 4 * 4, 4096, _IDX
        if fold2:
            d.a2_scale, d.a2_shift, d.a2_act, d.a2_slope = _SC, _SH, H.ACT_LRELU, 0.2
    return d


def _plan(H, L, d):
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


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("M", [592, 20480, 327680])
def test_supported_plan_is_the_ordinary_layers(lib, mode, M):
    H, L = lib
    assert L.rl_set_wide_gemm(mode.encode()) == 0
    launches = L.rl_launch_count()
    for N, K, split in ((128, 128, 64), (128, 256, 128), (64, 128, 64), (256, 128, 64)):
        rc0, plain = _plan(H, L, _desc(H, M, N, K))
        assert rc0 == OK and plain[2] == b"pwgrad128w_kernel" and plain[1] == 512
        for fold2 in (True, False):
            d = _desc(H, M, N, K, split, fold2=fold2)
            rc, got = _plan(H, L, d)
            assert rc == OK, L.rl_last_error()
            assert got == plain
            assert L.rl_wgrad_batchable(C.byref(d)) == L.rl_wgrad_batchable(C.byref(_desc(H, M, N, K))) == 1
    assert L.rl_launch_count() == launches


UNSUPPORTED = {
    # name: (mode, N, K, split, rows_bf16)
    "fp32 arithmetic mode (pwgrad128_kernel)": ("fp32", 128, 128, 64, 0),
    "bf16 rows, bf16x3": ("bf16x3", 128, 128, 64, 1),
    "bf16 rows, bf16": ("bf16", 128, 128, 64, 1),
    "K = 3 * split": ("bf16x3", 128, 192, 64, 0),
    "K = 4 * split": ("bf16x3", 128, 256, 64, 0),
    "K = 2 * split - 16": ("bf16x3", 128, 112, 64, 0),
    "split 24": ("bf16x3", 128, 48, 24, 0),
    "split 60": ("bf16x3", 128, 120, 60, 0),
    "split 72": ("bf16", 128, 144, 72, 0),
    "the streaming kernel's shapes": ("bf16x3", 32, 32, 16, 0),
    "the streaming kernel's shapes, 64": ("bf16x3", 64, 64, 32, 0),
}


@pytest.mark.parametrize("name", sorted(UNSUPPORTED))
def test_everything_else_is_unsupported_and_launches_nothing(lib, name):
    H, L = lib
    mode, N, K, split, rows_bf16 = UNSUPPORTED[name]
    assert L.rl_set_wide_gemm(mode.encode()) == 0
    launches = L.rl_launch_count()
    for M in (592, 327680):
        d = _desc(H, M, N, K, split, rows_bf16)
        rc, _ = _plan(H, L, d)
        assert rc == ERR_UNSUPPORTED, (name, M, rc, L.rl_last_error())
        assert L.rl_last_error().startswith(b"rl_wgrad:")
        assert L.rl_wgrad_batchable(C.byref(d)) == 0
    assert L.rl_launch_count() == launches


def test_malformed_second_source_is_an_argument_error(lib):
    H, L = lib
    assert L.rl_set_wide_gemm(b"bf16x3") == 0
    for edit in (dict(A2=None), dict(a2_idx=None), dict(a2_bstride=0), dict(a2_shift=None), dict(A2=_A2 + 4), dict(lda2=62),
                 dict(lda2=60), dict(a2_split=128), dict(a2_split=-16), dict(a_mode=1)):
        d = _desc(H, 20480, 128, 128, 64)
        for k, v in edit.items():
            setattr(d, k, v)
        rc, _ = _plan(H, L, d)
        assert rc == ERR_ARGS, (edit, rc)


def test_setter_round_trip():
    from randlanet import _hip as H
    L = H.lib()
    mode0 = L.rl_get_pool128_x()
    try:
        assert mode0 in (b"in_place", b"stored")
        for m in (b"stored", b"in_place"):
            assert L.rl_set_pool128_x(m) == 0 and L.rl_get_pool128_x() == m
        assert L.rl_set_pool128_x(b"sometimes") == ERR_ARGS and L.rl_set_pool128_x(None) == ERR_ARGS
        assert L.rl_get_pool128_x() == b"in_place"
    finally:
        L.rl_set_pool128_x(mode0)
