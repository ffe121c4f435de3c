"""Every kernel instantiation plan_gemm / plan_wgrad can return, on the MI355X, against fp64 - elementwise.

One case per row of tests/gemm_lattice.py.  A case applies the row's process settings (restored in a `finally`), and at each M
edge of the row launches through ops.gemm / ops.wgrad, asserts that the plan of the very descriptor launched (rl_gemm_plan /
rl_wgrad_plan2) is the row's and that rl_last_kernel names it, and holds the result to the derived elementwise bound of the
module's docstring - the statistics, dbias and BatchNorm-backward sums to the project's own tolerances, and everything outside
the product (rows beyond n of a batch-strided Y, columns beyond N, the other destination of a split) to bit-for-bit silence.
The largest error / bound per kernel family and arithmetic is printed when the module is done.
"""
import numpy as np
import pytest
import torch

import gemm_lattice as G

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from randlanet import _ops
    return _ops


@pytest.fixture(scope="module")
def H():
    from randlanet import _hip
    return _hip


@pytest.fixture(scope="module")
def report():
    worst = {}
    yield worst
    for (family, arith), (ratio, where) in sorted(worst.items()):
        print(f"[gemm lattice] {family:<20} {arith:<7} max error / bound {ratio:.3f}  ({where})")


def _note(report, case, ratio, where):
    key = (case.family, case.arith)
    if ratio >= report.get(key, (-1.0, ""))[0]:
        report[key] = (ratio, where)


def _operand(ops, inp):
    c, o, t, B, n = inp.case, inp.opts, inp.t, inp.B, inp.n
    act = o.lazy if o.lazy is not None else 0

    def lazy(raw, rows, C, scale, shift):
        bs = raw.shape[0] // B
        if scale is None:
            return ops.Lazy(raw, B, rows, bs, C)
        return ops.Lazy(raw, B, rows, bs, C, scale, shift, act, G.SLOPE if act == 2 else 0.0)

    if c.operand == "rpe":
        return ops.Rpe(t["xyz"], t["nbr_idx"], t["nbr_d2"], B, n, t["nbr_idx"].shape[2])
    if c.operand == "cat":
        h = c.K // 2
        u = lazy(t["U"], n, h, t.get("u_scale"), t.get("u_shift"))
        g = lazy(t["G"], t["G"].shape[0] // B - 2, h, t.get("g_scale"), t.get("g_shift"))
        return ops.InterpConcat(g, u, t["idx"]) if c.a2_first else ops.ConcatGather(u, g, t["idx"])
    return lazy(t["A"], n, c.K, t.get("scale"), t.get("shift"))


def _untouched(full, before, B, rows, cols):
    """Everything of `full` outside the first `rows` rows of each cloud and the first `cols` columns holds `before`'s bits."""
    mask = torch.ones(full.shape, dtype=torch.bool, device=full.device)
    mask.view(B, -1, full.shape[1])[:, :rows, :cols] = False
    return torch.equal(full.view(torch.int32)[mask], before.view(torch.int32)[mask])


def _gemm_edge(ops, H, report, case, i, j, M):
    inp = G.make_inputs(case, i, j, M, DEV)
    t, o, B, K, N = inp.t, inp.opts, inp.B, case.K, case.N
    rows = M // B                                   # rows per cloud
    a = _operand(ops, inp)
    W = t["W"]
    ks, ns = (N, 1) if o.w_n_contig else (1, K)
    ws = ops.split_weights([(W, ks, ns, K, N, True)]) if case.planes else None
    assert not case.planes or ws, "the row needs pre-split planes"
    Y = t["Y0"].clone()
    ybs = Y.shape[0] // B
    kw = {}
    stats = None
    if case.stats:
        stats = torch.full((H.MAX_SLOTS, 2, N), float("nan"), dtype=torch.float64, device=DEV)
        kw["stats"] = stats
        if "piv_mean" in t:
            kw["pivot"] = (t["piv_mean"], t.get("piv_bias"))
    out2 = None
    if "addend" in t:
        kw["addend"] = t["addend"]
    if "out2_0" in t:
        out2 = t["out2_0"].clone()
        kw.update(out2=out2, split_col=case.split_col)
    bnb = None
    if case.epilogue == "bnb":
        act = G.bnb_act(i, j)
        bnb = ops.Lazy(t["bnb_Y"], B, rows, ybs, N, t["bnb_scale"], t["bnb_shift"], act, G.SLOPE if act == 2 else 0.0, t["bnb_mean"],
                       t["bnb_invstd"], "x")
        kw["bnb"] = bnb
    plan = {}
    res = ops.gemm(a, W, ks, ns, N, t.get("bias"), out=Y, out_bstride=ybs, accumulate=o.accumulate, wsplit=ws, plan=plan, **kw)
    last = H.lib().rl_last_kernel().decode()
    G.plan_matches(case, plan, M)
    assert last == case.kernel, (case.id, M, last)
    where = f"{case.id} M={M}"
    ref, env = G.reference_gemm(inp)
    coef = G.coefficient(case.arith, K)
    ycols = case.split_col if out2 is not None else N
    Yl = Y.view(B, ybs, -1)[:, :rows, :ycols].reshape(M, ycols)
    ratio = G.check(Yl, ref[:, :ycols], env[:, :ycols], coef, where)
    if out2 is not None:
        ratio = max(ratio, G.check(out2, ref[:, ycols:], env[:, ycols:], coef, where + " (out2)"))
    _note(report, case, ratio, where)
    assert _untouched(Y, t["Y0"], B, rows, ycols), f"{where}: rl_gemm wrote outside the product"
    Yd = Yl.double()
    if stats is not None:
        nslots = ops.gemm_stat_slots(M, N, K)
        piv = 0.0
        if "piv_mean" in t:
            piv = (t["piv_mean"] - t["piv_bias"] if "piv_bias" in t else t["piv_mean"]).double()
        s = stats[:nslots]
        np.testing.assert_allclose(s[:, 0].sum(0).cpu().numpy(), (Yd - piv).sum(0).cpu().numpy(), rtol=1e-5, atol=1e-4, err_msg=where)
        np.testing.assert_allclose(s[:, 1].sum(0).cpu().numpy(), ((Yd - piv) ** 2).sum(0).cpu().numpy(), rtol=1e-5, atol=1e-4, err_msg=where)
    if bnb is not None:
        pre = res[1]
        assert pre is not None, f"{where}: the streaming kernel should have left the BatchNorm-backward sums"
        tl = t["bnb_Y"].view(B, ybs, -1)[:, :rows, :N].reshape(M, N)
        z = tl * t["bnb_scale"] + t["bnb_shift"]                      # (fp32, two roundings: the kernel's own expression)
        neg = 0.0 if bnb.act == 1 else (G.SLOPE if bnb.act == 2 else 1.0)
        gp = Yd * torch.where(z > 0, 1.0, neg).double()
        xhat = (tl.double() - t["bnb_mean"].double()) * t["bnb_invstd"].double()
        want = torch.stack([gp.sum(0), (gp * xhat).sum(0)])
        got = pre[0][:pre[1]].sum(0)
        scale_s = float(want.abs().max()) + 1e-6
        assert float((got - want).abs().max()) < 2e-5 * scale_s + 1e-4, (where, got, want)


def _wgrad_edge(ops, H, report, case, i, j, M):
    inp = G.make_inputs(case, i, j, M, DEV)
    t, o, B, K, N = inp.t, inp.opts, inp.B, case.K, case.N
    a = _operand(ops, inp)
    dY = t["dY"]
    dW = torch.full((K, N) if o.w_n_contig else (N, K), 7.0, device=DEV)
    ks, ns = (N, 1) if o.w_n_contig else (1, K)
    db = torch.full((N,), 7.0, device=DEV) if o.dbias else None
    plan = {}
    ops.wgrad(a, dY, dY.shape[0] // B, N, dW, ks, ns, db, plan=plan)
    last = H.lib().rl_last_kernel().decode()
    G.plan_matches(case, plan, M)
    assert last == case.kernel, (case.id, M, last)
    where = f"{case.id} M={M}"
    ref, env, colsum = G.reference_wgrad(inp)
    ratio = G.check(dW if o.w_n_contig else dW.t(), ref, env, G.coefficient(case.arith, M), where)
    _note(report, case, ratio, where)
    if db is not None:
        assert float((db.double() - colsum).abs().max()) <= 1e-5 * M, where


@pytest.mark.parametrize("i", range(len(G.CASES)), ids=[c.id for c in G.CASES])
def test_lattice_row(ops, H, report, i):
    case = G.CASES[i]
    L = H.lib()
    mode0 = L.rl_get_wide_gemm()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    try:
        G.apply_settings(L, case)
        for j, M in enumerate(G.case_Ms(case, cus)):
            (_gemm_edge if case.op == "gemm" else _wgrad_edge)(ops, H, report, case, i, j, M)
    finally:
        G.restore_settings(L, mode0)
