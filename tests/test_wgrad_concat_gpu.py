"""Level-2 pooling backward without a stored X: the wide weight gradient reads X's two halves in place.

Kernel level: dW and the partial slabs of rl_wgrad / rl_wgrad_batch with the concat-gather operand (U, G, idx) are those of
the same calls on the X that rl_pool_bwd stores, bit for bit, in the bf16x3 and the bf16 arithmetic mode; both are reported
against an fp64 X^T.dS (the stored-X path's error is the yardstick).  Pooling kernel: with rl_pool_desc.x_optional and no
X_out, GU / DG / dS_out are those of the storing launch and memory that was not passed stays untouched.  Step level: one
TrainStep with a 128-wide level, eager and replayed, gives the same gradient, weights, record and logits either way.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
D, HALF = 128, 64


def _inputs(B, n, g_act, seed):
    """One d = 128 pooling block: U rows, a per-point table G given as a prefix view (bstride > n), idx with 0, n - 1 and
    repeats, folds whose pre-activations are negative about half the time in both halves."""
    from randlanet import _hip as H
    from randlanet import _ops as ops
    g = torch.Generator().manual_seed(seed)
    P, gb = B * n, n + 5
    u_raw = torch.randn((P * 16, HALF), generator=g)
    g_raw = torch.randn((B * gb, HALF), generator=g)
    fold = lambda: (torch.empty(HALF).uniform_(-1.5, 1.5, generator=g), torch.empty(HALF).uniform_(-0.5, 0.5, generator=g))
    (u_sc, u_sh), (g_sc, g_sh) = fold(), fold()
    idx = torch.randint(0, n, (B, n, 16), generator=g, dtype=torch.int32)
    idx[:, :, 0] = 0
    idx[:, :, 5] = n - 1
    idx[:, :, 7] = idx[:, :, 6]
    idx[:, 0, :] = n - 1
    idx[:, n - 1, :] = 0
    W = torch.randn((D, D), generator=g) * 0.1
    dP = torch.randn((P, D), generator=g)
    to = lambda t: t.to(DEV).contiguous()
    u = ops.Lazy(to(u_raw), B, n * 16, n * 16, HALF, to(u_sc), to(u_sh), H.ACT_RELU, 0.0)
    gl = ops.Lazy(to(g_raw), B, n, gb, HALF, to(g_sc), to(g_sh), g_act, 0.2 if g_act == H.ACT_LRELU else 0.0)
    return u, gl, to(idx), to(W), to(dP)


def _pool_bwd(u, g, idx, W, dP, n, store_x, flag):
    """rl_pool_bwd at d = 128 through the descriptor; returns (X or None, dS, GU, DG)."""
    from randlanet import _hip as H
    from randlanet import _ops as ops
    P = u.B * n
    pd = ops._pool_desc(u, g, idx, W, n, D)
    new = lambda c: torch.empty((P * 16, c), dtype=torch.float32, device=DEV)
    X, dS, GU, DG = (new(D) if store_x else None), new(D), new(HALF), new(HALF)
    dW = torch.empty(D * D, device=DEV)
    pd.dP, pd.GU, pd.gu_accumulate, pd.DG, pd.dW = dP.data_ptr(), GU.data_ptr(), 0, DG.data_ptr(), dW.data_ptr()
    pd.X_out, pd.dS_out, pd.x_optional = (X.data_ptr() if store_x else None), dS.data_ptr(), int(flag)
    rc = H.lib().rl_pool_bwd(C.byref(pd), H.stream_ptr())
    return rc, X, dS, GU, DG


def _x_reference(u, g, idx, n):
    """X = [act(bn(U)) | act(bn(G[idx]))] in torch, fp32 and un-fused like the kernels."""
    from randlanet import _hip as H
    act = lambda z, a, s: torch.relu(z) if a == H.ACT_RELU else torch.where(z > 0, z, z * s)
    left = act(u.raw * u.scale + u.shift, u.act, u.slope)
    gv = g.raw.view(g.B, g.bstride, HALF)
    rows = torch.stack([gv[b][idx[b].reshape(-1).long()] for b in range(g.B)]).reshape(-1, HALF)
    return torch.cat([left, act(rows * g.scale + g.shift, g.act, g.slope)], dim=1)


def _wgrad_both_ways(a, dS, n):
    """(dW, slabs) of rl_wgrad and of rl_wgrad_batch + rl_wgrad_reduce_batch for the operand a."""
    from randlanet import _hip as H
    from randlanet import _ops as ops
    M = dS.shape[0]
    nsplit, per = H.lib().rl_wgrad_nsplit(M, D, D), D * D + D
    out = []
    dW = torch.zeros(D * D, device=DEV)
    ops.wgrad(a, dS, n * 16, D, dW, 1, D, None)
    slab = ops._slab(DEV, nsplit * per)[:nsplit * per].view(nsplit, per)[:, :D * D].clone()
    out.append((dW, slab))
    dW2 = torch.zeros(D * D, device=DEV)
    pending, batch = [], []
    ops.wgrad(a, dS, n * 16, D, dW2, 1, D, None, pending=pending, batch=batch)
    assert len(batch) == 1 and batch[0][6] == 1, "the layer must join the grouped launch of the wide kernel"
    slab2 = pending[0][1]
    ops.wgrad_batch_flush(batch)
    assert H.lib().rl_last_kernel() == b"pwgrad128w_batch_kernel"
    ops.wgrad_flush(pending)
    out.append((dW2, slab2[:nsplit * per].view(nsplit, per)[:, :D * D].clone()))
    return out, nsplit


@pytest.fixture(scope="module")
def blocks():
    """Inputs and the storing pooling launch per case and arithmetic mode, computed once: {(case, mode): dict}."""
    from randlanet import _hip as H
    from randlanet import _ops as ops
    cases = {"ragged": (1, 37, H.ACT_RELU, 11), "split": (2, 640, H.ACT_LRELU, 12)}
    mode0 = ops.get_wide_gemm()
    out = {}
    try:
        for name, (B, n, g_act, seed) in cases.items():
            u, g, idx, W, dP = _inputs(B, n, g_act, seed)
            for mode in ("bf16x3", "bf16"):
                ops.set_wide_gemm(mode)
                rc, X, dS, GU, DG = _pool_bwd(u, g, idx, W, dP, n, store_x=True, flag=0)
                assert rc == 0, H.lib().rl_last_error()
                torch.cuda.synchronize()
                out[(name, mode)] = dict(B=B, n=n, u=u, g=g, idx=idx, W=W, dP=dP, X=X, dS=dS, GU=GU, DG=DG)
    finally:
        ops.set_wide_gemm(mode0)
    return out


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("case", ["ragged", "split"])
def test_weight_gradient_from_the_two_sources_equals_the_stored_x(blocks, case, mode):
    from randlanet import _ops as ops
    k = blocks[(case, mode)]
    B, n, u, g, idx, X, dS = k["B"], k["n"], k["u"], k["g"], k["idx"], k["X"], k["dS"]
    assert (B * n * 16) % 32 != 0 if case == "ragged" else True
    assert torch.equal(X, _x_reference(u, g, idx, n)), "the stored X is not [act(bn(U)) | act(bn(G[idx]))]"
    assert float((X[:, :HALF] == 0).float().mean()) > 0.2 and float((X[:, HALF:] <= 0).float().mean()) > 0.2
    mode0 = ops.get_wide_gemm()
    try:
        ops.set_wide_gemm(mode)
        stored, nsplit = _wgrad_both_ways(ops.plain(X, B, n * 16), dS, n)
        two, _ = _wgrad_both_ways(ops.ConcatGather(u, g, idx), dS, n)
        torch.cuda.synchronize()
    finally:
        ops.set_wide_gemm(mode0)
    assert nsplit > 1 if case == "split" else nsplit >= 1
    ref = (dS.double().t() @ X.double()).reshape(-1)        # dW[o][i] = sum_r dS[r][o] X[r][i]
    for entry, (dw_s, slab_s), (dw_t, slab_t) in zip(("rl_wgrad", "rl_wgrad_batch"), stored, two):
        err_s, err_t = float((dw_s.double() - ref).abs().max()), float((dw_t.double() - ref).abs().max())
        print(f"{case} {mode} {entry}: nsplit {nsplit}, |dW| max {float(ref.abs().max()):.3e}, error against fp64: stored X "
              f"{err_s:.3e}, two sources {err_t:.3e}")
        assert torch.equal(slab_t, slab_s), f"{entry}: partial slabs differ"
        assert torch.equal(dw_t, dw_s), f"{entry}: dW differs"
        assert err_t <= err_s
    assert torch.equal(stored[0][0], stored[1][0]) and torch.equal(two[0][0], two[1][0])


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("case", ["ragged", "split"])
def test_pooling_backward_without_x_out(blocks, case, mode):
    from randlanet import _hip as H
    from randlanet import _ops as ops
    k = blocks[(case, mode)]
    n, u, g, idx, W, dP = k["n"], k["u"], k["g"], k["idx"], k["W"], k["dP"]
    mode0 = ops.get_wide_gemm()
    try:
        ops.set_wide_gemm(mode)
        sentinel = torch.full_like(k["X"], -12345.0)
        rc, X, dS, GU, DG = _pool_bwd(u, g, idx, W, dP, n, store_x=False, flag=1)
        assert rc == 0, H.lib().rl_last_error()
        assert H.lib().rl_last_kernel() == b"pool128_bwd_kernel"
        torch.cuda.synchronize()
        assert torch.equal(dS, k["dS"]) and torch.equal(GU, k["GU"]) and torch.equal(DG, k["DG"])
        assert bool((sentinel == -12345.0).all())
        # the flag makes X_out optional, not forbidden
        rc, X, dS, GU, DG = _pool_bwd(u, g, idx, W, dP, n, store_x=True, flag=1)
        assert rc == 0, H.lib().rl_last_error()
        torch.cuda.synchronize()
        assert torch.equal(X, k["X"]) and torch.equal(dS, k["dS"]) and torch.equal(GU, k["GU"]) and torch.equal(DG, k["DG"])
        # without the flag the call is refused as before, and nothing is launched
        launches = H.lib().rl_launch_count()
        rc, *_ = _pool_bwd(u, g, idx, W, dP, n, store_x=False, flag=0)
        assert rc == H.ERR_ARGS and H.lib().rl_launch_count() == launches
    finally:
        ops.set_wide_gemm(mode0)


def test_unsupported_settings_launch_nothing(blocks):
    """Exact-fp32 arithmetic keeps the stored-X path: the two-source operand is refused by rl_wgrad and rl_wgrad_batch."""
    from randlanet import _hip as H
    from randlanet import _ops as ops
    k = blocks[("ragged", "bf16x3")]
    a = ops.ConcatGather(k["u"], k["g"], k["idx"])
    mode0 = ops.get_wide_gemm()
    try:
        ops.set_wide_gemm("fp32")
        assert not ops.wgrad_supported(a, k["dS"], k["n"] * 16, D)
        launches = H.lib().rl_launch_count()
        with pytest.raises(H.HipKernelError):
            ops.wgrad(a, k["dS"], k["n"] * 16, D, torch.zeros(D * D, device=DEV), 1, D, None)
        assert H.lib().rl_launch_count() == launches
        ops.set_wide_gemm("bf16x3")
        assert ops.wgrad_supported(a, k["dS"], k["n"] * 16, D)
    finally:
        ops.set_wide_gemm(mode0)


def test_train_step_is_the_same_either_way(monkeypatch):
    """layers [16, 64, 128]: level 2 pools at d = 128.  Two steps (the second one's forward sees the first one's gradients),
    eager and replayed: gradient, weights, loss record and the logits of a further forward are equal between the settings."""
    from randlanet import _ops as ops
    from randlanet._train import TrainStep
    from randlanet.utils.modules import RandLANet, RandLANetSettings
    Cn, K, layers, B, N = 3, 16, [16, 64, 128], 2, 1024
    rs = np.random.RandomState(0)
    x = rs.uniform(0, 1, (B, N, 3)).astype(np.float32)
    y = np.floor(x[..., 2] * Cn).clip(0, Cn - 1).astype(np.int64)
    perms = [rs.permutation(N) for _ in range(3)]
    mode0 = ops.get_pool128_x()
    got, widths, pool_bwd = {}, [], ops.pool_bwd

    def counted(u, g, idx, W, n, d, *a, **kw):
        widths.append(d)
        return pool_bwd(u, g, idx, W, n, d, *a, **kw)

    monkeypatch.setattr(ops, "pool_bwd", counted)
    try:
        for setting in ("stored", "in_place"):
            ops.set_pool128_x(setting)
            for graph in (False, True):
                torch.manual_seed(0)
                net = RandLANet(RandLANetSettings(n_classes=Cn, n_points=N, n_neighbors=K, layer_sizes=layers), DEV)
                net.fc_end[2].p = 0.0
                net.train()
                step = TrainStep(net, B, N, loss="dice", lr=1e-2, use_graph=graph)
                step.set_batch(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
                step.capture()
                for p in perms[:2]:
                    step.step(p)
                torch.cuda.synchronize()
                rec = step.out.clone()
                grad, param = step.flat.grad.clone(), step.flat.param.detach().clone()
                perm = torch.from_numpy(perms[2]).to(DEV)
                logits, ctx = step.engine.forward(step.inp, perm, True, 0.0)
                logits = logits.clone()
                ctx.tape.clear()
                ctx.keep.clear()
                torch.cuda.synchronize()
                got[(setting, graph)] = (grad, param, rec, logits)
    finally:
        ops.set_pool128_x(mode0)
    assert 128 in widths, "the network has no 128-wide pooling level"
    base = got[("stored", False)]
    assert torch.isfinite(base[0]).all() and float(base[0].abs().max()) > 0
    for key, val in got.items():
        for what, a, b in zip(("gradient", "weights", "record", "logits"), val, base):
            assert torch.equal(a, b), (key, what)


@pytest.mark.parametrize("N,split,u_fold", [(128, 16, False), (64, 128, True), (128, 64, False)])
def test_other_splits_and_a_cloud_boundary_inside_a_chunk(N, split, u_fold):
    """The plan supports every K = 2 * split with 16 | split: split 16 (most lanes of the tile idle), split 128 (two k tiles, the
    second one gathered as a whole) and 64 once more, here with 304 rows per cloud - cloud boundaries fall inside 32-row chunks -
    three clouds, and a source 1 without a fold.  X is built in torch and handed over as a plain operand for the yardstick."""
    from randlanet import _hip as H
    from randlanet import _ops as ops
    g = torch.Generator().manual_seed(100 + split)
    B, rows, n_g, gb = 3, 304, 50, 57
    M, K = B * rows, 2 * split
    to = lambda t: t.to(DEV).contiguous()
    fold = lambda: (to(torch.empty(split).uniform_(-1.5, 1.5, generator=g)), to(torch.empty(split).uniform_(-0.5, 0.5, generator=g)))
    u_raw, g_raw = to(torch.randn((M, split), generator=g)), to(torch.randn((B * gb, split), generator=g))
    idx = torch.randint(0, n_g, (M,), generator=g, dtype=torch.int32)
    idx[::7], idx[3::11] = 0, n_g - 1
    idx = to(idx)
    dY = to(torch.randn((M, N), generator=g))
    u = ops.Lazy(u_raw, B, rows, rows, split, *(fold() if u_fold else (None, None)), H.ACT_RELU if u_fold else H.ACT_NONE, 0.0)
    gl = ops.Lazy(g_raw, B, n_g, gb, split, *fold(), H.ACT_LRELU, 0.2)
    left = torch.relu(u_raw * u.scale + u.shift) if u_fold else u_raw
    cloud = torch.arange(M, device=DEV) // rows
    z = g_raw[cloud * gb + idx.long()] * gl.scale + gl.shift
    X = torch.cat([left, torch.where(z > 0, z, z * 0.2)], dim=1).contiguous()

    def run(a):
        dW, pending, batch = torch.zeros(N * K, device=DEV), [], []
        ops.wgrad(a, dY, rows, N, dW, 1, K, None, pending=pending, batch=batch)
        assert len(batch) == 1 and batch[0][6] == 1
        ops.wgrad_batch_flush(batch)
        ops.wgrad_flush(pending)
        dW1 = torch.zeros(N * K, device=DEV)
        ops.wgrad(a, dY, rows, N, dW1, 1, K, None)
        return dW, dW1

    stored, two = run(ops.plain(X, B, rows)), run(ops.ConcatGather(u, gl, idx))
    torch.cuda.synchronize()
    ref = (dY.double().t() @ X.double()).reshape(-1)
    for entry, s, t in zip(("rl_wgrad_batch", "rl_wgrad"), stored, two):
        err_s, err_t = float((s.double() - ref).abs().max()), float((t.double() - ref).abs().max())
        print(f"N {N} K {K} split {split} {entry}: error against fp64: stored X {err_s:.3e}, two sources {err_t:.3e}")
        assert torch.equal(t, s), entry
        assert err_t <= err_s
