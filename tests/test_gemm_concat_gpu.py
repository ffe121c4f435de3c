"""The score product and the attentive pooling of an un-fused pooling block without a stored X.

rl_gemm with the concat-gather A operand (rl_gemm_desc.a2_*: U, G, idx) against rl_copy_rows_pair into a stored X followed by
rl_gemm on it, and rl_attpool_fwd_cat / rl_attpool_bwd_cat against rl_attpool_fwd / rl_attpool_bwd on that X, in one process:
every comparison is torch.equal.  The in-place operand has to have the bits of the stored copy (max(z, z*e): a clipped ReLU
input is -0) and the arithmetic behind the load is the same in the same order, so nothing may differ.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _sources(B, n, split, u_fold, g_fold, seed, pad=True):
    """U rows (B * n * 16, split) with ReLU, the per-point table G as a prefix view (bstride > n) of wider rows (lda2 > C) with
    LeakyReLU 0.2, idx with 0, n - 1 and repeats; folds whose pre-activations are negative about half the time."""
    from randlanet import _hip as H
    from randlanet import _ops as ops
    g = torch.Generator().manual_seed(seed)
    rows, gb, ldg = B * n * 16, n + (5 if pad else 0), split + (8 if pad else 0)
    to = lambda t: t.to(DEV).contiguous()
    u_raw = torch.randn((rows, split), generator=g)
    g_raw = torch.randn((B * gb, ldg), generator=g)
    fold = lambda on: (to(torch.empty(split).uniform_(-1.5, 1.5, generator=g)), to(torch.empty(split).uniform_(-0.5, 0.5, generator=g))) if on else (None, None)
    idx = torch.randint(0, n, (B, n, 16), generator=g, dtype=torch.int32)
    idx[:, :, 0] = 0
    idx[:, :, 5] = n - 1
    idx[:, :, 7] = idx[:, :, 6]
    idx[:, 0, :] = n - 1
    idx[:, n - 1, :] = 0
    u = ops.Lazy(to(u_raw), B, n * 16, n * 16, split, *fold(u_fold), H.ACT_RELU if u_fold else H.ACT_NONE, 0.0)
    gl = ops.Lazy(to(g_raw), B, n, gb, split, *fold(g_fold), H.ACT_LRELU if g_fold else H.ACT_NONE, 0.2 if g_fold else 0.0)
    return u, gl, to(idx)


def _stored_x(u, g, idx):
    from randlanet import _ops as ops
    rows, h, rpc = u.rows, u.C, u.n
    X = torch.empty((rows, 2 * h), dtype=torch.float32, device=DEV)
    ops.copy_rows_pair(((u.raw, (0, h), rpc, X, (0, h), rows, rpc), dict(lazy=u)),
                       ((g.raw, (0, h), g.bstride, X, (h, h), rows, rpc), dict(index=idx, lazy=g)))
    return X


def _x_reference(u, g, idx):
    from randlanet import _hip as H
    act = lambda z, a, s: torch.relu(z) if a == H.ACT_RELU else torch.where(z > 0, z, z * s) if a == H.ACT_LRELU else z
    h = u.C
    left = act(u.raw * u.scale + u.shift, u.act, u.slope) if u.scale is not None else u.raw
    gv = g.raw.view(g.B, g.bstride, -1)[:, :, :h]
    rows = torch.stack([gv[b][idx[b].reshape(-1).long()] for b in range(g.B)]).reshape(-1, h)
    right = act(rows * g.scale + g.shift, g.act, g.slope) if g.scale is not None else rows
    return torch.cat([left, right], dim=1)


def _weights(K, N, seed):
    from randlanet import _ops as ops
    W = (torch.randn((N, K), generator=torch.Generator().manual_seed(seed)) * 0.1).to(DEV)
    return W, ops.split_weights([(W, 1, K, K, N)])


# B = 3, n = 36: 576 rows per cloud - cloud boundaries fall inside 64-row and 128-row tiles - and M = 1728, so the last tile
# of either height is half full.  B = 2, n = 640: 20480 rows, 128 x 128 tiles, at ny = 2 some persistent workgroups own two tiles.
CASES = {
    # name: (B, n, split, N, u_fold, g_fold)
    "score product, split 64": (3, 36, 64, 128, True, True),
    "score product, split 128": (3, 36, 128, 256, True, True),
    "several tiles per workgroup": (2, 640, 128, 256, True, True),
    "source 1 without a fold": (3, 36, 128, 256, False, True),
    "source 2 without a fold": (3, 36, 64, 128, True, False),
}


@pytest.fixture(scope="module")
def cases():
    out = {}
    for i, (name, (B, n, split, N, uf, gf)) in enumerate(CASES.items()):
        u, g, idx = _sources(B, n, split, uf, gf, 40 + i)
        X = _stored_x(u, g, idx)
        W, planes = _weights(2 * split, N, 70 + i)
        out[name] = dict(B=B, n=n, split=split, N=N, u=u, g=g, idx=idx, X=X, W=W, planes=planes)
    torch.cuda.synchronize()
    return out


@pytest.fixture()
def settings():
    from randlanet import _ops as ops
    mode0 = ops.get_wide_gemm()
    yield ops
    ops.set_wide_gemm(mode0)
    ops.set_wgemm_tile("auto")


@pytest.mark.parametrize("tile", ["auto", "64x128", "64x64"])
@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_product_from_the_two_sources_equals_the_stored_x(cases, settings, case, mode, tile):
    from randlanet import _hip as H
    ops = settings
    k = cases[case]
    B, n, split, N, u, g, idx, X, W = k["B"], k["n"], k["split"], k["N"], k["u"], k["g"], k["idx"], k["X"], k["W"]
    K = 2 * split
    assert torch.equal(X, _x_reference(u, g, idx)), "the stored X is not [act(bn(U)) | act(bn(G[idx]))]"
    if u.scale is not None:
        assert float((X[:, :split] == 0).float().mean()) > 0.2
    ops.set_wide_gemm(mode)
    ops.set_wgemm_tile(tile)
    a = ops.ConcatGather(u, g, idx)
    assert ops.gemm_concat_supported(a, W, 1, K, N, k["planes"])
    Ys = ops.gemm(ops.plain(X, B, n * 16), W, 1, K, N, None, wsplit=k["planes"])
    assert H.lib().rl_last_kernel() == b"wgemm2_kernel"
    Yt = ops.gemm(a, W, 1, K, N, None, wsplit=k["planes"])
    assert H.lib().rl_last_kernel() == b"wgemm2_kernel<cat>"      # (wgemm2_cat_kernel: not the ordinary instantiation)
    torch.cuda.synchronize()
    ref = X.double() @ W.double().t()
    err_s, err_t = float((Ys.double() - ref).abs().max()), float((Yt.double() - ref).abs().max())
    print(f"{case} {mode} {tile}: M {X.shape[0]} K {K} N {N}, |Y| max {float(ref.abs().max()):.3e}, error against fp64: stored X "
          f"{err_s:.3e}, two sources {err_t:.3e}")
    assert torch.isfinite(Yt).all() and float(Yt.abs().max()) > 0
    assert torch.equal(Yt, Ys)


@pytest.mark.parametrize("case", ["score product, split 128", "several tiles per workgroup"])
def test_statistics_are_the_stored_operands(cases, settings, case):
    ops = settings
    k = cases[case]
    B, n, split, N, X, W = k["B"], k["n"], k["split"], k["N"], k["X"], k["W"]
    K, M = 2 * split, X.shape[0]
    ops.set_wide_gemm("bf16x3")
    slots = ops.gemm_stat_slots(M, N, K)
    st_s, st_t = ops.new_stats(DEV, N).fill_(-1.0), ops.new_stats(DEV, N).fill_(-2.0)
    Ys = ops.gemm(ops.plain(X, B, n * 16), W, 1, K, N, None, wsplit=k["planes"], stats=st_s)
    Yt = ops.gemm(ops.ConcatGather(k["u"], k["g"], k["idx"]), W, 1, K, N, None, wsplit=k["planes"], stats=st_t)
    torch.cuda.synchronize()
    assert torch.equal(Yt, Ys)
    assert torch.equal(st_t[:slots], st_s[:slots])
    # folded: column sums and sums of squares over all slots
    tot = st_t[:slots].sum(dim=0)
    ref = torch.stack([Ys.double().sum(dim=0), (Ys.double() ** 2).sum(dim=0)])
    assert torch.allclose(tot, ref, rtol=1e-5, atol=1e-6 * M)
    assert bool((st_t[slots:] == -2.0).all()), "slots beyond rl_gemm_stat_slots were written"


def test_accumulate_and_untouched_neighbours(cases, settings):
    """accumulate adds into Y; memory behind the last row of Y stays untouched when the last tile is half full."""
    ops = settings
    k = cases["score product, split 128"]
    B, n, split, N, X, W = k["B"], k["n"], k["split"], k["N"], k["X"], k["W"]
    K, M = 2 * split, X.shape[0]
    ops.set_wide_gemm("bf16x3")
    base = torch.randn((M + 64, N), generator=torch.Generator().manual_seed(5)).to(DEV)
    out_s, out_t = base.clone(), base.clone()
    ops.gemm(ops.plain(X, B, n * 16), W, 1, K, N, None, wsplit=k["planes"], out=out_s, accumulate=True)
    ops.gemm(ops.ConcatGather(k["u"], k["g"], k["idx"]), W, 1, K, N, None, wsplit=k["planes"], out=out_t, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(out_t, out_s) and torch.equal(out_t[M:], base[M:]) and not torch.equal(out_t[:M], base[:M])


def test_unsupported_settings_launch_nothing(cases, settings):
    from randlanet import _hip as H
    ops = settings
    k = cases["score product, split 128"]
    a = ops.ConcatGather(k["u"], k["g"], k["idx"])
    K, N = 2 * k["split"], k["N"]
    for change in ("fp32", "registers", "no planes"):
        try:
            if change == "fp32":
                ops.set_wide_gemm("fp32")
            if change == "registers":
                ops.set_wgemm_staging("registers")
            planes = None if change == "no planes" else k["planes"]
            assert not ops.gemm_concat_supported(a, k["W"], 1, K, N, planes), change
            launches = H.lib().rl_launch_count()
            with pytest.raises(H.HipKernelError):
                ops.gemm(a, k["W"], 1, K, N, None, wsplit=planes)
            assert H.lib().rl_launch_count() == launches
        finally:
            ops.set_wide_gemm("bf16x3")
            ops.set_wgemm_staging("dma")
    assert ops.gemm_concat_supported(a, k["W"], 1, K, N, k["planes"])


# ---- attentive pooling: P = 108 (B = 3, n = 36) and P = 1280 (B = 2, n = 640), C = 256 ------------------------------------------
@pytest.mark.parametrize("case", ["score product, split 128", "several tiles per workgroup", "source 1 without a fold"])
def test_attentive_pooling_from_the_two_sources(cases, case):
    from randlanet import _hip as H
    from randlanet import _ops as ops
    k = cases[case]
    B, n, X = k["B"], k["n"], k["X"]
    P, Cc = B * n, X.shape[1]
    assert Cc == 256 and P in (108, 1280)
    g = torch.Generator().manual_seed(9)
    S = (torch.randn((P * 16, Cc), generator=g) * 2).to(DEV)
    dP = torch.randn((P, Cc), generator=g).to(DEV)
    a = ops.ConcatGather(k["u"], k["g"], k["idx"])
    assert ops.attpool_concat_supported(a, P, 16) and not ops.attpool_concat_supported(a, P // 2, 32)
    pooled_s = ops.attpool_fwd(X, S, P, 16)
    pooled_t = ops.attpool_fwd(a, S, P, 16)
    assert H.lib().rl_last_kernel() == b"attpool_fwd_kernel"
    dS_s, dXa_s = ops.attpool_bwd(X, S, pooled_s, dP, P, 16)
    dS_t, dXa_t = ops.attpool_bwd(a, S, pooled_s, dP, P, 16)
    torch.cuda.synchronize()
    A = torch.softmax(S.double().view(P, 16, Cc), dim=1)
    ref = (A * X.double().view(P, 16, Cc)).sum(dim=1)
    print(f"{case}: P {P}, pooled error against fp64: stored X {float((pooled_s.double() - ref).abs().max()):.3e}, two sources "
          f"{float((pooled_t.double() - ref).abs().max()):.3e}")
    assert torch.isfinite(pooled_t).all() and float(dS_t.abs().max()) > 0
    assert torch.equal(pooled_t, pooled_s)
    assert torch.equal(dS_t, dS_s)
    assert torch.equal(dXa_t, dXa_s)
    # bytes too: the sign of a zero in dS depends on the sign of a zero in X
    assert torch.equal(dS_t.view(torch.int32), dS_s.view(torch.int32))


def test_bf16_rows_are_refused_where_fp32_rows_are_taken(cases, settings):
    """The storage type is the one rule rl_gemm_desc cannot express: ops.gemm_concat_supported takes the fp32 sources of a case
    and refuses the same sources with either half in bf16."""
    ops = settings
    k = cases["score product, split 128"]
    u, g, idx, W = k["u"], k["g"], k["idx"], k["W"]
    ops.set_wide_gemm("bf16x3")
    assert ops.gemm_concat_supported(ops.ConcatGather(u, g, idx), W, 1, 256, 256, k["planes"]) is True
    as_bf16 = lambda z: ops.Lazy(z.raw.to(torch.bfloat16), z.B, z.n, z.bstride, z.C, z.scale, z.shift, z.act, z.slope)
    for uu, gg in ((as_bf16(u), g), (u, as_bf16(g)), (as_bf16(u), as_bf16(g))):
        assert ops.gemm_concat_supported(ops.ConcatGather(uu, gg, idx), W, 1, 256, 256, k["planes"]) is False
