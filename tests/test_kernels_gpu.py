"""Kernel-level parity on the MI355X: every C-ABI entry point against the oracle (KNN, losses)
or a plain PyTorch fp32 statement of the same op.  Tolerances are written at each assert."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
os.environ.setdefault("RL_ALLOW_FLOAT_ATOMICS", "1")     # the two non-deterministic (fp32-atomic) entry points are tested too

from knn_parity import check_knn  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    from randlanet import _ops
    return _ops


@pytest.fixture(scope="module")
def H():
    from randlanet import _hip
    return _hip


DEV = "cuda"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------ KNN
def _golden_cases(golden_dir):
    z = np.load(f"{golden_dir}/knn_cases.npz")
    for t in sorted({k.split("/")[0] for k in z.files if k.endswith("/idx")}):
        data = str(z[f"{t}/data"])
        sup = z[f"{data}/support"]
        qry = z[f"{data}/query"] if f"{data}/query" in z.files else sup
        yield t, sup, qry, int(z[f"{t}/k"]), z[f"{t}/idx"], z[f"{t}/d2"]


def test_knn_golden_reference_vectors(ops, golden_dir):
    """HIP KNN vs outputs of the reference's own knn_tpk.knn: d2 bit-exact, idx tie-aware."""
    for tag, sup, qry, k, ref_idx, ref_d2 in _golden_cases(golden_dir):
        idx, d2 = ops.knn_f32(_t(sup[None]), _t(qry[None]), k)
        frac = check_knn(idx[0].cpu().numpy(), d2[0].cpu().numpy(), ref_idx, ref_d2, sup, qry,
                         expect_lowest_index=True)
        if tag.startswith(("uniform", "cross")):
            assert frac == 1.0, tag


@pytest.mark.parametrize("B,Ns,Nq,k", [(2, 5000, 3000, 16), (1, 2049, 1025, 32), (3, 700, 700, 1),
                                        (1, 64, 10, 64), (2, 1500, 1500, 5)])
def test_knn_matches_oracle_bitwise(ops, B, Ns, Nq, k):
    from oracle import randlanet_oracle as O
    rs = np.random.RandomState(Ns + k)
    s = rs.normal(0, 1, (B, Ns, 3)).astype(np.float32)
    q = rs.normal(0, 1, (B, Nq, 3)).astype(np.float32)
    ri, rd = O.knn(torch.from_numpy(s), torch.from_numpy(q), k, "grid")
    idx, d2 = ops.knn_f32(_t(s), _t(q), k)
    assert torch.equal(idx.cpu(), ri) and torch.equal(d2.cpu().view(torch.int32), rd.view(torch.int32))
    i32, d2b = ops.knn_i32(_t(s), _t(q), Ns, Nq, k)
    assert torch.equal(i32.cpu().long(), ri) and torch.equal(d2b.cpu(), rd)


def _clouds():
    rs = np.random.RandomState(7)
    yield "uniform", rs.uniform(0, 1, (2, 3000, 3)).astype(np.float32)
    yield "clustered", (rs.normal(0, 1, (2, 3000, 3)) ** 3).astype(np.float32)
    yield "planar", np.concatenate([rs.uniform(0, 1, (1, 2500, 2)), np.full((1, 2500, 1), 0.25)], -1).astype(np.float32)
    line = np.zeros((1, 2048, 3), np.float32)
    line[0, :, 1] = rs.uniform(-5, 5, 2048)
    yield "collinear", line
    yield "identical", np.full((1, 1500, 3), 0.75, np.float32)
    g = np.arange(12, dtype=np.float32)
    yield "lattice", np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(1, -1, 3)
    dup = rs.uniform(0, 1, (1, 40, 3)).astype(np.float32)[:, rs.randint(0, 40, 2500)]
    yield "duplicates", dup


@pytest.mark.parametrize("k", [1, 16, 32])
def test_knn_grid_equals_brute_force_on_hard_clouds(ops, k):
    """The uniform-grid search (supports >= 1024 points) and the tiled scan give the same bits,
    in self-search mode (queries walked in cell order) and for foreign queries, including
    queries far outside the support's bounding box."""
    for name, pts in _clouds():
        x = _t(pts)
        bi, bd = ops.knn_i32(x, x, pts.shape[1], pts.shape[1], k, brute=True)
        gi, gd = ops.knn_i32(x, x, pts.shape[1], pts.shape[1], k)                 # self mode
        assert torch.equal(bi, gi) and torch.equal(bd, gd), (name, "self")
        rs = np.random.RandomState(3)
        q = _t((pts[:, :777] + rs.normal(0, 0.3, pts[:, :777].shape)).astype(np.float32) * 1.7 - 0.4)
        bi, bd = ops.knn_i32(x, q, pts.shape[1], 777, k, brute=True)
        gi, gd = ops.knn_i32(x, q, pts.shape[1], 777, k)
        assert torch.equal(bi, gi) and torch.equal(bd, gd), (name, "cross")


def test_knn_multi_equals_single_searches(ops):
    """rl_knn_multi (all searches of a forward in one launch set) gives the bits of the one-by-one calls."""
    rs = np.random.RandomState(11)
    xyz = _t(rs.uniform(0, 1, (3, 4096, 3)).astype(np.float32))
    tasks = [(4096, 4096, 16), (1024, 1024, 16), (256, 256, 16), (64, 64, 16), (16, 64, 1), (64, 256, 1),
             (256, 1024, 1), (1024, 4096, 1), (4096, 4096, 5), (300, 4000, 32)]          # 10 tasks -> two chunks
    got = ops.knn_multi(xyz, tasks)
    assert len(got) == len(tasks)
    for (Ns, Nq, k), (idx, d2) in zip(tasks, got):
        ri, rd = ops.knn_i32(xyz, xyz, Ns, Nq, k, brute=True)
        assert torch.equal(idx, ri) and torch.equal(d2, rd), (Ns, Nq, k)


def test_knn_prefix_strides_and_errors(ops, H):
    from oracle import randlanet_oracle as O
    rs = np.random.RandomState(1)
    xyz = rs.uniform(0, 1, (2, 4096, 3)).astype(np.float32)
    # the network searches prefixes of the permuted cloud in place (modules.py:587-598)
    i32, d2 = ops.knn_i32(_t(xyz), _t(xyz), 1024, 4096, 1)
    ri, rd = O.knn(torch.from_numpy(xyz[:, :1024].copy()), torch.from_numpy(xyz), 1)
    assert torch.equal(i32.cpu().long(), ri) and torch.equal(d2.cpu(), rd)
    assert torch.equal(i32[:, :1024, 0].cpu(), torch.arange(1024, dtype=torch.int32).expand(2, -1))
    with pytest.raises(H.HipKernelError, match="Not enough points"):
        ops.knn_f32(_t(xyz[:, :3]), _t(xyz[:, :3]), 4)
    with pytest.raises(H.HipKernelError, match="RL_KNN_MAX_K"):
        ops.knn_f32(_t(xyz), _t(xyz), 65)
    idx, d2 = ops.knn_f32(_t(xyz), _t(xyz[:, :0]), 3)       # empty query set
    assert idx.shape == (2, 0, 3)


def test_knn_full_size_properties(ops):
    """Config A size (N=40960, K=16): properties that need no oracle run."""
    rs = np.random.RandomState(2)
    xyz = _t(rs.uniform(0, 1, (2, 40960, 3)).astype(np.float32))
    idx, d2 = ops.knn_i32(xyz, xyz, 40960, 40960, 16)
    assert int(idx.min()) >= 0 and int(idx.max()) < 40960
    assert bool((d2[..., 1:] >= d2[..., :-1]).all())
    assert torch.equal(idx[..., 0], torch.arange(40960, device=DEV, dtype=torch.int32).expand(2, -1))
    assert float(d2[..., 0].abs().max()) == 0.0
    g = torch.gather(xyz, 1, idx.long().reshape(2, -1, 1).expand(-1, -1, 3)).reshape(2, 40960, 16, 3)
    diff = xyz[:, :, None, :] - g
    chk = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
    assert torch.equal(chk, d2)
    # a 2048-query sample against the oracle
    from oracle import randlanet_oracle as O
    ri, rd = O.knn(xyz[:1].cpu(), xyz[:1, :2048].cpu().contiguous(), 16)
    assert torch.equal(idx[0, :2048].cpu().long(), ri[0]) and torch.equal(d2[0, :2048].cpu(), rd[0])


# ----------------------------------------------------------------------------------- GEMM
def _act(z, act, slope):
    if act == 1:
        return torch.relu(z)
    if act == 2:
        return torch.nn.functional.leaky_relu(z, slope)
    return z


@pytest.mark.parametrize("B,n,K,N,transposed,lazy,bias", [
    (2, 1000, 3, 8, False, False, True),       # fc_start shape (K not a multiple of 4)
    (2, 3000, 8, 16, False, True, True),
    (1, 517, 16, 16, False, False, False),     # score Linear, no bias
    (2, 777, 64, 32, False, True, True),
    (3, 130, 128, 256, False, True, True),
    (2, 160, 512, 512, False, True, True),     # bottleneck
    (2, 640, 1024, 256, True, False, True),    # decoder.0 ConvTranspose2d
    (2, 999, 64, 8, True, True, True),
    (1, 300, 32, 2, False, True, True),        # fc_end.3
    (1, 300, 32, 13, False, False, True),
])
def test_gemm_forward(ops, B, n, K, N, transposed, lazy, bias):
    torch.manual_seed(K * N + n)
    A = torch.randn(B * n, K, device=DEV)
    W = torch.randn((K, N) if transposed else (N, K), device=DEV) / K ** 0.5
    b = torch.randn(N, device=DEV) if bias else None
    a = ops.plain(A, B, n)
    ref_in = A
    if lazy:
        a.scale, a.shift = torch.rand(K, device=DEV) + 0.5, torch.randn(K, device=DEV) * 0.3
        a.act, a.slope = 2, 0.2
        ref_in = _act(A * a.scale + a.shift, 2, 0.2)
    ks, ns = ops.weight_strides(W, transposed, K, N)
    stats = ops.new_stats(DEV, N)
    Y = ops.gemm(a, W, ks, ns, N, b, stats=stats)
    Wm = W if transposed else W.t()
    ref = ref_in.double() @ Wm.double() + (b.double() if bias else 0)
    tol = 2e-6 * K ** 0.5 * float(ref.abs().max()) + 1e-6   # exact-fp32 FMA chain vs fp64
    assert float((Y.double() - ref).abs().max()) <= tol
    nslots = ops.gemm_stat_slots(B * n, N, K)
    s = stats[:nslots]
    np.testing.assert_allclose(s[:, 0].sum(0).cpu().numpy(), Y.double().sum(0).cpu().numpy(), rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(s[:, 1].sum(0).cpu().numpy(), (Y.double() ** 2).sum(0).cpu().numpy(), rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("M,K,N", [(3000, 128, 128), (700, 512, 256), (1500, 96, 192)])
def test_wide_gemm_modes(ops, M, K, N):
    """fp32 MFMA vs the default bf16x3 split vs plain bf16, forward / dgrad-style operand / weight gradient, against fp64."""
    torch.manual_seed(M)
    A = torch.randn(M, K, device=DEV)
    W = torch.randn(N, K, device=DEV) / K ** 0.5
    Wt = W.t().contiguous()
    dY = torch.randn(M, N, device=DEV)
    ref = A.double() @ W.double().t()
    ref_w = dY.double().t() @ A.double()
    bound = {"fp32": 2e-6, "bf16x3": 4e-5, "bf16": 2e-2}     # relative to sqrt(K) * max|ref|: 2^-24, 2^-16, 2^-8 products
    initial = ops.get_wide_gemm()
    assert initial == os.environ.get("RL_WIDE_GEMM", "bf16x3")       # bf16x3 unless the environment chose another mode
    errs = {}
    try:
        for mode in ("fp32", "bf16x3", "bf16"):
            ops.set_wide_gemm(mode)
            assert ops.get_wide_gemm() == mode
            a = ops.plain(A, 1, M)
            Y = ops.gemm(a, W, 1, K, N)
            Y2 = ops.gemm(a, Wt, N, 1, N)                     # the same product through the n-contiguous weight path
            dW = torch.empty(N, K, device=DEV)
            ops.wgrad(a, dY, M, N, dW, 1, K, None)
            e = max(float((Y.double() - ref).abs().max()), float((Y2.double() - ref).abs().max())) / (K ** 0.5 * float(ref.abs().max()))
            ew = float((dW.double() - ref_w).abs().max()) / (M ** 0.5 * float(ref_w.abs().max()))
            errs[mode] = (e, ew)
            assert e < bound[mode] and ew < bound[mode], (mode, e, ew)
    finally:
        ops.set_wide_gemm(initial)
    assert errs["fp32"][0] < errs["bf16x3"][0] < errs["bf16"][0]
    with pytest.raises(Exception):
        ops.set_wide_gemm("fp16")


@pytest.mark.parametrize("d,B,n_parent,n,accumulate", [(128, 2, 500, 300, False), (256, 1, 400, 200, True)])
def test_gemm_split_scatter_epilogue(ops, d, B, n_parent, n, accumulate):
    """dX = addend + dS.W, first half stored / accumulated, second half scatter-added to the gathered rows, in one launch,
    against the three-launch composition (GEMM accumulate, copy_rows, scatter_add_rows)."""
    torch.manual_seed(d)
    K, h = 16, d // 2
    rows = B * n * K
    dS = torch.randn(rows, d, device=DEV)
    W = torch.randn(d, d, device=DEV) / d ** 0.5
    addend = torch.randn(rows, d, device=DEV)
    idx = torch.randint(0, n_parent, (B, n, K), device=DEV, dtype=torch.int32)
    gu0 = torch.randn(rows, h, device=DEV)
    # composition
    dX = addend.clone()
    ops.gemm(ops.plain(dS, B, n * K), W, d, 1, d, None, out=dX, out_bstride=n * K, accumulate=True)
    gu_ref = gu0.clone() if accumulate else torch.empty_like(gu0)
    ops.copy_rows(dX, (0, h), n * K, gu_ref, (0, h), rows, n * K, accumulate=accumulate)
    gg_ref = torch.zeros(B * n_parent, h, device=DEV)
    ops.scatter_add_rows(dX, (h, h), gg_ref, n_parent, rows, n * K, idx)
    # fused epilogue, atomic form (kept in the ABI)
    gu = gu0.clone() if accumulate else torch.full_like(gu0, float("nan"))
    gg = torch.zeros(B * n_parent, h, device=DEV)
    ops.gemm(ops.plain(dS, B, n * K), W, d, 1, d, None, out=gu, out_bstride=n * K, accumulate=accumulate,
             addend=addend, out2=gg, out2_index=idx.view(-1), out2_bstride=n_parent, split_col=h)
    # same products; the composition may have split K over workgroups (few row tiles), so the order can differ
    assert float((gu - gu_ref).abs().max()) < 1e-5 * float(gu_ref.abs().max())
    assert float((gg - gg_ref).abs().max()) < 1e-4 * float(gg_ref.abs().max())   # fp32 atomics: order differs
    # dense form + segment sum: what the network runs; bitwise reproducible
    (csr,) = ops.csr_build([(idx, n_parent)])
    res = []
    for _ in range(2):
        gu2 = gu0.clone() if accumulate else torch.full_like(gu0, float("nan"))
        DG = torch.full((rows, h), float("nan"), device=DEV)
        ops.gemm(ops.plain(dS, B, n * K), W, d, 1, d, None, out=gu2, out_bstride=n * K, accumulate=accumulate,
                 addend=addend, out2=DG, split_col=h)
        gg2 = torch.full((B * n_parent, h), float("nan"), device=DEV)
        ops.segment_sum_rows(DG, (0, h), n * K, csr, gg2, n_parent)
        res.append((gu2, gg2))
    assert torch.equal(res[0][0], gu) and torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert float((res[0][1] - gg_ref).abs().max()) < 1e-4 * float(gg_ref.abs().max())
    # narrow layers have no such epilogue: loud error, no silent fallback
    small = torch.randn(64, 32, device=DEV)
    with pytest.raises(Exception, match="split-scatter"):
        ops.gemm(ops.plain(small, 1, 64), torch.randn(32, 32, device=DEV), 32, 1, 32, None, out=torch.empty(64, 16, device=DEV),
                 addend=torch.zeros(64, 32, device=DEV), out2=torch.zeros(10, 16, device=DEV),
                 out2_index=torch.zeros(64, dtype=torch.int32, device=DEV), out2_bstride=10, split_col=16)


def test_gemm_asymmetric_identity(ops):
    """A = I with an asymmetric W catches a transposed C/D fragment map."""
    n = 128
    A = torch.eye(n, device=DEV)
    W = (torch.arange(n * 48, device=DEV, dtype=torch.float32).reshape(48, n) % 97) - 11.0   # (N,K)
    Y = ops.gemm(ops.plain(A, 1, n), W, 1, n, 48)
    assert torch.equal(Y, W.t().contiguous())


def test_gemm_batch_strided_accumulate(ops):
    torch.manual_seed(0)
    B, n_parent, n, K, N = 3, 400, 100, 32, 16
    A = torch.randn(B * n_parent, K, device=DEV)
    W = torch.randn(N, K, device=DEV)
    a = ops.Lazy(A, B, n, n_parent, K)
    out = torch.randn(B * n_parent, N, device=DEV)
    before = out.clone()
    ops.gemm(a, W, 1, K, N, None, out=out, out_bstride=n_parent, accumulate=True)
    Av = A.view(B, n_parent, K)[:, :n]
    ref = before.view(B, n_parent, N).clone()
    ref[:, :n] += Av @ W.t()
    assert float((out.view(B, n_parent, N) - ref).abs().max()) < 1e-4
    assert torch.equal(out.view(B, n_parent, N)[:, n:], before.view(B, n_parent, N)[:, n:])


def _rpe_ref(xyz, idx, d2):
    B, n, K = idx.shape
    xi = xyz[:, :n, None, :].expand(B, n, K, 3)
    xj = torch.gather(xyz, 1, idx.long().reshape(B, n * K, 1).expand(-1, -1, 3)).reshape(B, n, K, 3)
    return torch.cat([xi, xj, xi - xj, torch.sqrt(d2)[..., None]], -1).reshape(B * n * K, 10)


def test_gemm_rpe_source_and_wgrad(ops):
    torch.manual_seed(3)
    B, n_parent, n, K, N = 2, 600, 300, 16, 8
    xyz = torch.rand(B, n_parent, 3, device=DEV)
    idx, d2 = ops.knn_i32(xyz, xyz, n, n, K)
    W = torch.randn(N, 10, device=DEV)
    b = torch.randn(N, device=DEV)
    rpe = ops.Rpe(xyz, idx, d2, B, n, K)
    Y = ops.gemm(rpe, W, 1, 10, N, b)
    R = _rpe_ref(xyz, idx, d2)
    ref = R @ W.t() + b
    assert float((Y - ref).abs().max()) < 1e-5
    dY = torch.randn_like(Y)
    dW, db = torch.empty_like(W), torch.empty_like(b)
    ops.wgrad(rpe, dY, n * K, N, dW, 1, 10, db)
    assert float((dW - dY.t() @ R).abs().max()) < 2e-4 * float((dY.t() @ R).abs().max())
    assert float((db - dY.sum(0)).abs().max()) < 1e-3
    # the materialised encoding (rows x 12, two floats of padding) holds the same bits and gives the same layer
    T = ops.rpe_build(rpe)
    assert T.raw.shape == (B * n * K, 12) and T.C == 10
    assert torch.equal(T.raw[:, :9], R[:, :9]) and float(T.raw[:, 10:].abs().max()) == 0.0
    assert float((T.raw[:, 9] - R[:, 9]).abs().max()) < 1e-7          # torch's device sqrt is not correctly rounded
    Y2 = ops.gemm(T, W, 1, 10, N, b)
    assert float((Y2 - ref).abs().max()) < 1e-5
    dW2, db2 = torch.empty_like(W), torch.empty_like(b)
    ops.wgrad(T, dY, n * K, N, dW2, 1, 10, db2)
    assert float((dW2 - dY.t() @ R).abs().max()) < 2e-4 * float((dY.t() @ R).abs().max())
    assert float((db2 - dY.sum(0)).abs().max()) < 1e-3


@pytest.mark.parametrize("B,n,K,N,transposed,lazy", [
    (2, 5000, 8, 16, False, True), (1, 333, 16, 16, False, False), (2, 700, 64, 128, False, True),
    (2, 640, 1024, 256, True, False), (3, 257, 256, 512, False, True), (1, 4096, 32, 2, False, True),
    (2, 100, 3, 8, False, False),
])
def test_wgrad(ops, B, n, K, N, transposed, lazy):
    torch.manual_seed(n + K)
    A = torch.randn(B * n, K, device=DEV)
    dY = torch.randn(B * n, N, device=DEV)
    a = ops.plain(A, B, n)
    ref_in = A
    if lazy:
        a.scale, a.shift, a.act, a.slope = torch.rand(K, device=DEV) + 0.5, torch.randn(K, device=DEV), 1, 0.0
        ref_in = torch.relu(A * a.scale + a.shift)
    dW = torch.full((K, N) if transposed else (N, K), 7.0, device=DEV)
    db = torch.empty(N, device=DEV)
    ks, ns = ops.weight_strides(dW, transposed, K, N)
    ops.wgrad(a, dY, n, N, dW, ks, ns, db)
    ref = (ref_in.double().t() @ dY.double())           # (K,N)
    ref = ref if transposed else ref.t()
    tol = 3e-6 * (B * n) ** 0.5 * float(ref.abs().max()) + 1e-5
    assert float((dW.double() - ref).abs().max()) <= tol
    assert float((db.double() - dY.double().sum(0)).abs().max()) <= 1e-5 * B * n


# ------------------------------------------------------------------------------ BatchNorm
def test_wgrad_deferred_batch_reduce_is_bitwise_the_same(ops):
    """rl_wgrad(defer_reduce) + rl_wgrad_reduce_batch sums the same slabs in the same order as the per-layer reducer."""
    torch.manual_seed(11)
    shapes = [(2, 3000, 8, 16), (1, 700, 64, 128), (2, 640, 256, 128), (2, 500, 10, 8), (1, 900, 32, 2)] * 11   # 55 > 48 items
    pending, want, got = [], [], []
    for (B, n, K, N) in shapes:
        A = torch.randn(B * n, K, device=DEV)
        dY = torch.randn(B * n, N, device=DEV)
        a = ops.plain(A, B, n)
        dW0, db0 = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
        ops.wgrad(a, dY, n, N, dW0, 1, K, db0)
        dW1, db1 = torch.full((N, K), float("nan"), device=DEV), torch.full((N,), float("nan"), device=DEV)
        ops.wgrad(a, dY, n, N, dW1, 1, K, db1, pending=pending)
        want.append((dW0, db0)); got.append((dW1, db1))
    assert len(pending) == len(shapes)
    ops.wgrad_flush(pending)
    assert pending == []
    for (w0, b0), (w1, b1) in zip(want, got):
        assert torch.equal(w0, w1) and torch.equal(b0, b1)


@pytest.mark.parametrize("C,rows,one_launch", [(8, 5000, False), (64, 999, True), (64, 999, False), (512, 300, True), (1024, 257, True),
                                               (1024, 257, False), (64, 2048, True), (64, 2049, False)])
def test_bn_forward_backward(ops, C, rows, one_launch, monkeypatch):
    """one_launch: the backward of a small tensor is rl_bn_bwd_fused (one launch); otherwise reduce / finalize / apply."""
    monkeypatch.setattr(ops, "NO_BN_SMALL", not one_launch)
    assert bool(ops.H.lib().rl_bn_bwd_fused_supported(rows, C, C)) == (rows <= 2048)
    torch.manual_seed(C)
    Y = (torch.randn(rows, C, device=DEV) * 2 + 1).requires_grad_(True)
    gamma = (torch.rand(C, device=DEV) + 0.5).requires_grad_(True)
    beta = torch.randn(C, device=DEV).requires_grad_(True)
    rm, rv = torch.randn(C, device=DEV), torch.rand(C, device=DEV) + 0.5
    rm_ref, rv_ref = rm.clone(), rv.clone()
    nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
    # batch statistics come from a GEMM epilogue: run Y through an identity layer
    stats = ops.new_stats(DEV, C)
    eye = torch.eye(C, device=DEV)
    Yc = ops.gemm(ops.plain(Y.detach().contiguous(), 1, rows), eye, 1, C, C, None, stats=stats)
    # identity layer: exact on the fp32 MFMA kernels; the wide kernel's default arithmetic splits operands into bf16
    # head + tail (2^-17 relative representation error)
    assert torch.equal(Yc, Y.detach()) if C <= 64 else float((Yc - Y.detach()).abs().max()) < 2e-5 * float(Y.detach().abs().max())
    scale, shift, mean, invstd = ops.bn_finalize(stats, rows, 128, C, gamma.detach(), beta.detach(), rm, rv, nbt,
                                                 0.99, 1e-6, True)
    ref = torch.nn.functional.batch_norm(Y.t()[None], rm_ref, rv_ref, gamma, beta, True, 0.99, 1e-6)[0].t()
    out = Y.detach() * scale + shift
    assert float((out - ref.detach()).abs().max()) < 2e-5 * max(1.0, float(ref.detach().abs().max()))
    np.testing.assert_allclose(rm.cpu().numpy(), rm_ref.cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(rv.cpu().numpy(), rv_ref.cpu().numpy(), rtol=1e-4, atol=1e-6)
    assert int(nbt) == 1
    # backward through leaky_relu(bn(Y)): the reference is fp64 autograd of the same expression (torch's own fp32 batch_norm
    # backward is NOT usable as one on this ROCm build: against fp64 it is off by 3e-3 at 2047 rows, 7e-3 at 2049, 1.4 at 4097
    # for a (1, C, rows) input, while it is exact to 4e-7 at 2048 and 3000 - tools/micro/bn_dbg.py)
    Yd = Y.detach().double().requires_grad_(True)
    gd, bd = gamma.detach().double().requires_grad_(True), beta.detach().double().requires_grad_(True)
    refd = (Yd - Yd.mean(0)) / torch.sqrt(Yd.var(0, unbiased=False) + 1e-6) * gd + bd
    G = torch.randn(rows, C, device=DEV)
    torch.nn.functional.leaky_relu(refd, 0.2).backward(G.double())
    Y.grad, gamma.grad, beta.grad = Yd.grad.float(), gd.grad.float(), bd.grad.float()
    lz = ops.Lazy(Y.detach().contiguous(), 1, rows, rows, C, scale, shift, 2, 0.2, mean, invstd)
    g = G.clone()
    dgamma, dbeta = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    n0 = ops.H.lib().rl_launch_count()
    ops.bn_backward(g, lz, dgamma, dbeta, True)
    assert ops.H.lib().rl_launch_count() - n0 == (1 if one_launch else 3)
    sc = float(Y.grad.abs().max())
    assert float((g - Y.grad).abs().max()) < 1e-4 * sc + 1e-6
    np.testing.assert_allclose(dgamma.cpu().numpy(), gamma.grad.cpu().numpy(), rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose(dbeta.cpu().numpy(), beta.grad.cpu().numpy(), rtol=2e-4, atol=2e-3)
    # eval mode: scale/shift from running statistics
    s2, b2, _, _ = ops.bn_finalize(None, rows, 128, C, gamma.detach(), beta.detach(), rm, rv, None, 0.99, 1e-6, False)
    ref2 = torch.nn.functional.batch_norm(Y.detach().t()[None], rm, rv, gamma.detach(), beta.detach(), False, 0.99,
                                          1e-6)[0].t()
    assert float((Y.detach() * s2 + b2 - ref2).abs().max()) < 1e-5 * max(1.0, float(ref2.abs().max()))


@pytest.mark.parametrize("C,K,rows,fold", [(8, 3, 40000, True), (64, 64, 20000, False), (32, 16, 5001, True), (128, 128, 9000, True),
                                           (256, 64, 4097, False), (256, 512, 300, True), (64, 256, 2000, True)])
def test_shifted_batch_statistics(ops, C, K, rows, fold):
    """Round 5: BatchNorm batch statistics as SHIFTED sums (rl_gemm_desc.stats_pivot_*, rl_bn_finalize pivoted) - every GEMM
    kernel that leaves statistics (streaming, LDS-tiled wide, split-K reducer) on a layer whose channels have a spread of
    1e-4 of their mean: the reference's ATen BatchNorm is two-pass (modules.py:85-89), E[y^2] - E[y]^2 on fp32 partial sums
    loses such a variance altogether.  Against the fp64 statistics of the stored fp32 tensor: mean / invstd / running
    statistics with the pivot within 1e-4 relative; without it the same launch is off by orders of magnitude (printed)."""
    torch.manual_seed(C + K + rows)
    # Y = A.W: column k of A is ~1 with 1e-4 spread; W has one large positive entry per output -> channel mean ~100, spread ~1e-2
    A = (1.0 + 1e-4 * torch.randn(rows, K, device=DEV)).contiguous()
    W = torch.zeros(C, K, device=DEV)
    W[torch.arange(C), torch.arange(C) % K] = 100.0 + torch.arange(C, device=DEV, dtype=torch.float32) % 7
    bias = torch.randn(C, device=DEV) * 3
    gamma, beta = torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV)

    def run(pivot_on):
        rm = (W.sum(1) + bias + 0.05 * torch.randn(C, device=DEV)).contiguous()       # a running mean near the batch mean
        rv = torch.ones(C, device=DEV)
        rm0 = rm.clone()
        stats = ops.new_stats(DEV, C)
        Y = ops.gemm(ops.plain(A, 1, rows), W, 1, K, C, None if fold else bias, stats=stats,
                     pivot=(rm, bias if fold else None) if pivot_on else None)
        sc, sh, mean, invstd = ops.bn_finalize(stats, rows, 128, C, gamma, beta, rm, rv, None, 0.99, 1e-6, True,
                                               folded_bias=bias if fold else None, pivoted=pivot_on)
        return Y, mean, invstd, rm, rv, rm0

    Y, mean, invstd, rm, rv, rm0 = run(True)
    Yd = Y.double()
    m64, v64 = Yd.mean(0), Yd.var(0, unbiased=False)
    i64 = 1.0 / torch.sqrt(v64 + 1e-6)
    assert float(v64.max()) < 1e-3 and float(m64.abs().min()) > 50        # the regime this test is about
    e_mean = float(((mean.double() - m64).abs() / m64.abs()).max())
    e_inv = float(((invstd.double() - i64).abs() / i64).max())
    rm_ref = 0.01 * rm0.double() + 0.99 * (m64 + (bias.double() if fold else 0.0))
    rv_ref = 0.01 * 1.0 + 0.99 * v64 * rows / (rows - 1)
    _, _, inv_plain, _, _, _ = run(False)
    e_plain = float(((inv_plain.double() - i64).abs() / i64).max())
    print(f"[shifted statistics] C={C} K={K} rows={rows}: invstd error with the pivot {e_inv:.2e}, without {e_plain:.2e}")
    assert e_mean < 1e-6 and e_inv < 1e-4, (e_mean, e_inv)
    np.testing.assert_allclose(rm.cpu().numpy(), rm_ref.cpu().numpy(), rtol=1e-6)
    np.testing.assert_allclose(rv.cpu().numpy(), rv_ref.cpu().numpy(), rtol=2e-4, atol=1e-9)


# ----------------------------------------------------------------------------- rows, pool
@pytest.mark.parametrize("C,rows,one_launch", [(32, 5000, False), (128, 999, True), (512, 300, True), (512, 300, False), (32, 2048, True),
                                               (32, 2049, False)])
def test_residual_junction_bn_backward(ops, C, rows, one_launch, monkeypatch):
    """O = LeakyReLU_0.01(BN1(Y1) + BN2(Y2)) backward against torch autograd: two sweeps + the pair of folds, or - small tensors -
    ONE launch (rl_resid_bn_bwd_fused)."""
    monkeypatch.setattr(ops, "NO_BN_SMALL", not one_launch)
    torch.manual_seed(C + rows)
    Y = [(torch.randn(rows, C, device=DEV) * 1.5 + 0.3).requires_grad_(True) for _ in range(2)]
    gam = [(torch.rand(C, device=DEV) + 0.5).requires_grad_(True) for _ in range(2)]
    bet = [torch.randn(C, device=DEV).requires_grad_(True) for _ in range(2)]
    # reference: fp64 autograd of the same expression (see test_bn_forward_backward on torch's fp32 batch_norm backward here)
    Yd = [y.detach().double().requires_grad_(True) for y in Y]
    gd = [g.detach().double().requires_grad_(True) for g in gam]
    bd = [b.detach().double().requires_grad_(True) for b in bet]
    bn = [(Yd[i] - Yd[i].mean(0)) / torch.sqrt(Yd[i].var(0, unbiased=False) + 1e-6) * gd[i] + bd[i] for i in range(2)]
    O = torch.nn.functional.leaky_relu(bn[0] + bn[1], 0.01)
    G = torch.randn(rows, C, device=DEV)
    O.backward(G.double())
    O = O.float()
    for i in range(2):
        Y[i].grad, gam[i].grad, bet[i].grad = Yd[i].grad.float(), gd[i].grad.float(), bd[i].grad.float()
    lz = []
    for i in range(2):
        mean = Y[i].detach().mean(0)
        invstd = 1.0 / torch.sqrt(Y[i].detach().var(0, unbiased=False) + 1e-6)
        scale = gam[i].detach() * invstd
        lz.append(ops.Lazy(Y[i].detach().contiguous(), 1, rows, rows, C, scale, bet[i].detach() - mean * scale, 0, 0.0, mean, invstd))
    assert ops.resid_bn_supported(lz[0], lz[1])
    g = G.clone()
    dg = [torch.empty(C, device=DEV) for _ in range(4)]
    n0 = ops.H.lib().rl_launch_count()
    g2 = ops.resid_bn_backward(g, O.detach().contiguous(), 0.01, lz[0], lz[1], dg[0], dg[1], dg[2], dg[3])
    assert ops.H.lib().rl_launch_count() - n0 == (1 if one_launch else 3)
    for got, want in ((g, Y[0].grad), (g2, Y[1].grad)):
        assert float((got - want).abs().max()) < 1e-4 * float(want.abs().max()) + 1e-6
    np.testing.assert_allclose(dg[0].cpu().numpy(), gam[0].grad.cpu().numpy(), rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose(dg[1].cpu().numpy(), bet[0].grad.cpu().numpy(), rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose(dg[2].cpu().numpy(), gam[1].grad.cpu().numpy(), rtol=2e-4, atol=2e-3)
    np.testing.assert_allclose(dg[3].cpu().numpy(), bet[1].grad.cpu().numpy(), rtol=2e-4, atol=2e-3)
    assert not ops.resid_bn_supported(ops.Lazy(Y[0].detach()[:, :6].contiguous(), 1, rows, rows, 6, scale[:6], scale[:6], 0, 0.0, mean[:6], invstd[:6]),
                                      ops.Lazy(Y[1].detach()[:, :6].contiguous(), 1, rows, rows, 6, scale[:6], scale[:6], 0, 0.0, mean[:6], invstd[:6]))


def test_copy_rows_pair_equals_two_copies(ops):
    """rl_copy_rows_pair: the two halves of a concat in one launch (decoder concat modules.py:362, level-3 X = [rpe | gathered]
    modules.py:183) - bitwise what two rl_copy_rows calls leave, also on a shape the 16-byte path does not take."""
    torch.manual_seed(6)
    B, n_src, n, K = 2, 300, 170, 16
    for Ca, Cb in ((8, 24), (128, 128), (6, 8)):          # (6, 8): 6 % 4 != 0 -> the entry falls back to two launches
        U = torch.randn(B * n * K, Ca, device=DEV)
        src = torch.randn(B * n_src, Cb, device=DEV)
        idx = torch.randint(0, n_src, (B, n, K), device=DEV, dtype=torch.int32)
        lz = ops.Lazy(src, B, n, n_src, Cb, torch.rand(Cb, device=DEV) + 0.5, torch.randn(Cb, device=DEV), 1, 0.0)
        rows = B * n * K
        X1 = torch.zeros(rows, Ca + Cb, device=DEV)
        X2 = torch.zeros(rows, Ca + Cb, device=DEV)
        ops.copy_rows(U, (0, Ca), n * K, X1, (0, Ca), rows, n * K)
        ops.copy_rows(src, (0, Cb), n_src, X1, (Ca, Cb), rows, n * K, index=idx, lazy=lz)
        ops.copy_rows_pair(((U, (0, Ca), n * K, X2, (0, Ca), rows, n * K), {}),
                           ((src, (0, Cb), n_src, X2, (Ca, Cb), rows, n * K), dict(index=idx, lazy=lz)))
        assert torch.equal(X1, X2), (Ca, Cb)


def test_copy_rows_gather_concat_scatter(ops):
    torch.manual_seed(5)
    B, n_src, n, K, Cc = 2, 500, 200, 16, 8
    src = torch.randn(B * n_src, Cc, device=DEV)
    idx = torch.randint(0, n, (B, n, K), device=DEV, dtype=torch.int32)
    lz = ops.Lazy(src, B, n, n_src, Cc, torch.rand(Cc, device=DEV) + 0.5, torch.randn(Cc, device=DEV), 2, 0.2)
    U = torch.randn(B * n * K, Cc, device=DEV)
    X = torch.empty(B * n * K, 2 * Cc, device=DEV)
    ops.copy_rows(U, (0, Cc), n * K, X, (0, Cc), B * n * K, n * K)
    ops.copy_rows(src, (0, Cc), n_src, X, (Cc, Cc), B * n * K, n * K, index=idx, lazy=lz)
    act = torch.nn.functional.leaky_relu(src * lz.scale + lz.shift, 0.2).view(B, n_src, Cc)
    g = torch.gather(act, 1, idx.long().reshape(B, n * K, 1).expand(-1, -1, Cc)).reshape(B * n * K, Cc)
    assert torch.equal(X[:, :Cc], U) and float((X[:, Cc:] - g).abs().max()) < 1e-6
    # shared permutation index (int64), as for the input permutation (modules.py:571-573)
    perm = torch.randperm(n_src, device=DEV)
    out = torch.empty(B * n_src, Cc, device=DEV)
    ops.copy_rows(src, (0, Cc), n_src, out, (0, Cc), B * n_src, n_src, index=perm, index_shared=True)
    assert torch.equal(out.view(B, n_src, Cc), src.view(B, n_src, Cc)[:, perm])
    # 3-channel rows (scalar path): the xyz permutation
    xyz = torch.randn(B * n_src, 3, device=DEV)
    out3 = torch.empty_like(xyz)
    ops.copy_rows(xyz, (0, 3), n_src, out3, (0, 3), B * n_src, n_src, index=perm, index_shared=True)
    assert torch.equal(out3.view(B, n_src, 3), xyz.view(B, n_src, 3)[:, perm])
    # transposed movement: gradient of the gather
    dX = torch.randn(B * n * K, 2 * Cc, device=DEV)
    dG = torch.zeros(B * n_src, Cc, device=DEV)
    ops.scatter_add_rows(dX, (Cc, Cc), dG, n_src, B * n * K, n * K, idx)
    ref = torch.zeros(B, n_src, Cc, device=DEV)
    ref.scatter_add_(1, idx.long().reshape(B, n * K, 1).expand(-1, -1, Cc), dX[:, Cc:].reshape(B, n * K, Cc))
    assert float((dG.view(B, n_src, Cc) - ref).abs().max()) < 1e-4
    # accumulate into a column range
    acc = torch.ones(B * n * K, Cc, device=DEV)
    ops.copy_rows(dX, (0, Cc), n * K, acc, (0, Cc), B * n * K, n * K, accumulate=True)
    assert torch.equal(acc, 1 + dX[:, :Cc])
    # the quad path moves four chunks per lane and trip: odd sizes (tails of every length), ReLU / no activation, gather +
    # lazy + accumulate at once
    for rows_n, Cw, act in ((1, 4, 1), (3, 8, 0), (257, 12, 1), (1031, 64, 2)):
        srcw = torch.randn(B * n_src, Cw, device=DEV)
        ix = torch.randint(0, n_src, (B, rows_n), device=DEV, dtype=torch.int32)
        lzw = ops.Lazy(srcw, B, rows_n, n_src, Cw, torch.rand(Cw, device=DEV) + 0.5, torch.randn(Cw, device=DEV), act, 0.1)
        outw = torch.full((B * rows_n, Cw), 2.0, device=DEV)
        ops.copy_rows(srcw, (0, Cw), n_src, outw, (0, Cw), B * rows_n, rows_n, index=ix, lazy=lzw, accumulate=True)
        z = srcw * lzw.scale + lzw.shift
        a = z if act == 0 else (torch.relu(z) if act == 1 else torch.nn.functional.leaky_relu(z, 0.1))
        refw = 2.0 + torch.gather(a.view(B, n_src, Cw), 1, ix.long().view(B, rows_n, 1).expand(-1, -1, Cw)).reshape(B * rows_n, Cw)
        assert float((outw - refw).abs().max()) < 1e-6, (rows_n, Cw, act)


@pytest.mark.parametrize("P,K,Cc", [(1000, 16, 16), (300, 32, 64), (77, 16, 256), (50, 5, 10)])
def test_attpool(ops, P, K, Cc):
    torch.manual_seed(P)
    X = torch.randn(P * K, Cc, device=DEV, requires_grad=True)
    S = (torch.randn(P * K, Cc, device=DEV) * 2).requires_grad_(True)
    out = ops.attpool_fwd(X.detach(), S.detach(), P, K)
    A = torch.softmax(S.view(P, K, Cc), dim=1)
    ref = (A * X.view(P, K, Cc)).sum(1)
    assert float((out - ref).abs().max()) < 1e-5
    dP = torch.randn(P, Cc, device=DEV)
    ref.backward(dP)
    dS, dXa = ops.attpool_bwd(X.detach(), S.detach(), out, dP, P, K)
    assert float((dS - S.grad).abs().max()) < 1e-5 and float((dXa - X.grad).abs().max()) < 1e-5


@pytest.mark.parametrize("d,B,n_parent,n", [(16, 2, 700, 300), (32, 1, 257, 257), (64, 3, 400, 130), (128, 2, 300, 150)])
def test_fused_pool_forward_backward(ops, d, B, n_parent, n):
    """rl_pool_fwd / rl_pool_bwd against a plain PyTorch statement of gather + concat + score Linear +
    softmax over K + weighted sum (modules.py:213-221, 246-253) and its autograd."""
    if not ops.pool_supported(d, 16):
        assert d == 128 and ops.get_wide_gemm() == "fp32"      # the 128-channel kernels exist in the bf16 modes only
        pytest.skip("d = 128 fused pooling needs the bf16x3 / bf16 arithmetic mode")
    torch.manual_seed(d + n)
    K, h = 16, d // 2
    U = torch.randn(B * n * K, h, device=DEV)
    Gf = torch.randn(B * n_parent, h, device=DEV)
    idx = torch.randint(0, n, (B, n, K), device=DEV, dtype=torch.int32)
    W = (torch.randn(d, d, device=DEV) / d ** 0.5).requires_grad_(True)
    us, ub = torch.rand(h, device=DEV) + 0.5, torch.randn(h, device=DEV) * 0.3
    gs, gb = torch.rand(h, device=DEV) + 0.5, torch.randn(h, device=DEV) * 0.3
    u = ops.Lazy(U, B, n * K, n * K, h, us, ub, 1, 0.0)
    g = ops.Lazy(Gf, B, n, n_parent, h, gs, gb, 2, 0.2)
    # reference with autograd on the ACTIVATED operands
    ua = torch.relu(U * us + ub).requires_grad_(True)
    ga = torch.nn.functional.leaky_relu(Gf * gs + gb, 0.2).requires_grad_(True)
    gath = torch.gather(ga.view(B, n_parent, h), 1, idx.long().reshape(B, n * K, 1).expand(-1, -1, h)).reshape(B * n * K, h)
    X = torch.cat([ua, gath], 1)
    S = X @ W.t()
    A = torch.softmax(S.view(B * n, K, d), 1)
    Pref = (A * X.view(B * n, K, d)).sum(1)
    P = ops.pool_fwd(u, g, idx, W.detach(), n, d)
    assert float((P - Pref).abs().max()) < 2e-5
    dP = torch.randn(B * n, d, device=DEV)
    Pref.backward(dP)
    (csr,) = ops.csr_build([(idx, n)])
    GU = torch.full_like(U, 3.0)
    GG = torch.full_like(Gf, float("nan"))[: (B - 1) * n_parent + n]
    dW = torch.empty(d, d, device=DEV)
    DG = ops.pool_bwd(u, g, idx, W.detach(), n, d, dP, GU, False, dW)
    ops.segment_sum_rows(DG, (0, h), n * K, csr, GG, n_parent)                 # first writer: no zero fill
    GGv = torch.stack([GG[b * n_parent: b * n_parent + n] for b in range(B)])
    ref_gg = ga.grad.view(B, n_parent, h)[:, :n]
    assert float((GU - ua.grad).abs().max()) < 2e-5 * max(1.0, float(ua.grad.abs().max()))
    assert float((GGv - ref_gg).abs().max()) < 1e-4 * max(1.0, float(ga.grad.abs().max()))
    assert float((dW - W.grad).abs().max()) < 2e-4 * max(1.0, float(W.grad.abs().max()))
    GU2 = torch.ones_like(U)
    dW2 = torch.empty(d, d, device=DEV)
    DG2 = ops.pool_bwd(u, g, idx, W.detach(), n, d, dP, GU2, True, dW2)       # accumulate into GU
    assert float((GU2 - 1.0 - ua.grad).abs().max()) < 2e-5 * max(1.0, float(ua.grad.abs().max()))
    # no atomics anywhere: a second run gives the same bits
    GG2 = torch.empty_like(GG)
    ops.segment_sum_rows(DG2, (0, h), n * K, csr, GG2, n_parent)
    assert torch.equal(DG, DG2) and torch.equal(dW, dW2)
    assert torch.equal(GGv, torch.stack([GG2[b * n_parent: b * n_parent + n] for b in range(B)]))


@pytest.mark.parametrize("B,n_src,k,n_dst,Cc,kind", [(3, 500, 16, 500, 8, "uniform"), (2, 1000, 1, 250, 512, "uniform"),
                                                     (2, 300, 32, 300, 64, "uniform"), (1, 2500, 16, 2500, 32, "dup"),
                                                     (2, 200, 5, 77, 10, "uniform"), (1, 4096, 16, 4096, 16, "one"),
                                                     (2, 3000, 16, 3000, 8, "near"), (1, 2000, 4, 300000, 4, "uniform")])
def test_csr_transpose_and_segment_sum(ops, B, n_src, k, n_dst, Cc, kind):
    """rl_csr_build + rl_segment_sum_rows = the backward of torch.gather over a neighbour index, in a fixed order:
    segments hold exactly the gatherers of each point, ascending; sums equal scatter_add_ up to fp32 ordering; two
    runs are bitwise equal.  The last case (300000 destinations) is beyond the two-level sort's packing and takes the
    per-entry-atomics path.  "dup" / "one": duplicate-heavy graphs (predict.py's warm-up cloud, modules.py ties) where
    a few points are gathered by very many rows - the long-segment path."""
    torch.manual_seed(n_src + k)
    if kind == "uniform":
        idx = torch.randint(0, n_dst, (B, n_src, k), device=DEV, dtype=torch.int32)
    elif kind == "near":       # like a K-NN graph: row i gathers from i's surroundings (buckets see their own tiles' entries)
        idx = ((torch.arange(n_src, device=DEV).view(1, -1, 1) + torch.randint(-40, 41, (B, n_src, k), device=DEV)) % n_dst).to(torch.int32)
    elif kind == "dup":
        idx = torch.randint(0, 30, (B, n_src, k), device=DEV, dtype=torch.int32)        # 30 targets take everything
    else:
        idx = torch.zeros((B, n_src, k), device=DEV, dtype=torch.int32)
        idx[:, :, 1:] = 7                                                            # two segments of 4096 and 61440
    src = torch.randn(B * n_src * k, Cc + 4, device=DEV)
    outs = []
    for _ in range(2):
        (csr,) = ops.csr_build([(idx, n_dst)])
        dst = torch.full((B * n_dst + 3, Cc), float("nan"), device=DEV)
        ops.segment_sum_rows(src, (4, Cc), n_src * k, csr, dst, n_dst)
        outs.append((csr.offsets.clone(), csr.entries.clone(), dst[: B * n_dst].clone()))
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    off, ent, dst = (t.cpu() for t in outs[0])
    flat = idx.cpu().reshape(B, n_src * k).long()
    for b in range(B):
        order = torch.argsort(flat[b], stable=True)           # ascending source row inside every destination
        assert torch.equal(ent[b].long(), order)
        assert torch.equal(off[b].long(), torch.cat([torch.zeros(1, dtype=torch.long),
                                                     torch.bincount(flat[b], minlength=n_dst).cumsum(0)]))
    ref = torch.zeros(B, n_dst, Cc, dtype=torch.float64)
    ref.scatter_add_(1, flat.view(B, -1, 1).expand(-1, -1, Cc), src[:, 4:].cpu().double().view(B, n_src * k, Cc))
    assert float((dst.view(B, n_dst, Cc).double() - ref).abs().max()) < 1e-5 * max(1.0, float(ref.abs().max()))
    # accumulate
    acc = torch.ones(B * n_dst, Cc, device=DEV)
    (csr,) = ops.csr_build([(idx, n_dst)])
    ops.segment_sum_rows(src, (4, Cc), n_src * k, csr, acc, n_dst, accumulate=True)
    assert float((acc.cpu().view(B, n_dst, Cc).double() - 1.0 - ref).abs().max()) < 1e-5 * max(1.0, float(ref.abs().max()))


def test_add_act_and_logits_layout(ops):
    torch.manual_seed(9)
    rows, Cc = 1234, 32
    y1, y2 = torch.randn(rows, Cc, device=DEV), torch.randn(rows, Cc, device=DEV)
    l1 = ops.Lazy(y1, 1, rows, rows, Cc, torch.rand(Cc, device=DEV) + .5, torch.randn(Cc, device=DEV))
    l2 = ops.Lazy(y2, 1, rows, rows, Cc, torch.rand(Cc, device=DEV) + .5, torch.randn(Cc, device=DEV))
    O = ops.add_act_fwd(l1, l2, 0.01)
    ref = torch.nn.functional.leaky_relu((y1 * l1.scale + l1.shift) + (y2 * l2.scale + l2.shift), 0.01)
    assert float((O - ref).abs().max()) < 1e-6
    G = torch.randn_like(O)
    g = G.clone()
    ops.add_act_bwd(g, O, 0.01)
    assert torch.equal(g, torch.where(O > 0, G, G * 0.01))
    # a channel count that is not a multiple of four takes the scalar kernel; an odd number of quads the vector tail
    for rr, cw in ((77, 6), (3, 4), (1001, 20)):
        a1, a2 = torch.randn(rr, cw, device=DEV), torch.randn(rr, cw, device=DEV)
        m1 = ops.Lazy(a1, 1, rr, rr, cw, torch.rand(cw, device=DEV) + .5, torch.randn(cw, device=DEV))
        m2 = ops.Lazy(a2, 1, rr, rr, cw, torch.rand(cw, device=DEV) + .5, torch.randn(cw, device=DEV))
        o = ops.add_act_fwd(m1, m2, 0.2)
        r = torch.nn.functional.leaky_relu((a1 * m1.scale + m1.shift) + (a2 * m2.scale + m2.shift), 0.2)
        assert float((o - r).abs().max()) < 1e-6, (rr, cw)
    B, N, C = 2, 500, 3
    lp = torch.randn(B * N, C, device=DEV)
    perm = torch.randperm(N, device=DEV)
    logits = ops.logits_unpermute(lp, perm, B, N)
    ref = torch.empty(B, N, C, device=DEV)
    ref[:, perm] = lp.view(B, N, C)
    assert torch.equal(logits, ref.permute(0, 2, 1).contiguous())
    assert torch.equal(ops.logits_permute_grad(logits, perm), lp)


# ----------------------------------------------------------------------------- loss, adam
def test_loss_metrics_against_golden_and_oracle(ops, golden_dir):
    from oracle import loss_metrics_oracle as LM
    z = np.load(f"{golden_dir}/loss_metrics.npz")
    for tag in ("c2", "c5"):
        logits, labels = _t(z[f"{tag}/logits"]), _t(z[f"{tag}/labels"])
        C = logits.shape[1]
        for name, (kind, alpha, gamma) in ops.LOSS_KINDS.items():
            out, work = ops.loss_forward(logits, labels, kind, alpha, gamma, True)
            assert abs(float(out[0]) - float(z[f"{tag}/{name}"])) < 2e-6, (tag, name)     # vs the reference
            g = ops.loss_backward(logits, labels, kind, alpha, gamma, True, work)
            ref = z[f"{tag}/{name}_grad"]
            assert np.abs(g.cpu().numpy() - ref).max() < 1e-4 * np.abs(ref).max() + 1e-9, (tag, name)
        cnt = out[1:].cpu().numpy().reshape(4, C)
        inter, lab, pred = cnt[0], cnt[1], cnt[2]
        oa, pca = LM.accuracy(z[f"{tag}/logits"], z[f"{tag}/labels"])
        miou, pci = LM.iou(z[f"{tag}/logits"], z[f"{tag}/labels"])
        assert abs(inter.sum() / lab.sum() - oa) < 1e-7
        for c in range(C):
            union = lab[c] + pred[c] - inter[c]
            assert abs((1.0 if union == 0 else inter[c] / union) - pci[c]) < 1e-7
            assert abs((1.0 if lab[c] == 0 else inter[c] / lab[c]) - pca[c]) < 1e-7


def test_adam_matches_torch(ops):
    torch.manual_seed(1)
    n = 100003
    p = torch.randn(n, device=DEV)
    ref = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=1e-2)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    lr = torch.tensor([1e-2], device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    for it in range(4):
        g = torch.randn(n, device=DEV)
        ref.grad = g.clone()
        opt.step()
        ops.adam_step(p, g, m, v, lr, step)
    assert int(step) == 4
    assert float((p - ref.detach()).abs().max()) < 1e-6


@pytest.mark.parametrize("d,B,n_parent,n", [(16, 2, 900, 500), (32, 1, 300, 300), (64, 2, 400, 257)])
def test_virtual_rpe_branch_forward(ops, d, B, n_parent, n):
    """The rpe branch recomputed inside its consumers (rl_rpe_stats + rl_pool_fwd with u_source 1 / 2) against the
    same computation with the mlp_rpe1 / mlp_rpe2 outputs stored: BatchNorm batch statistics and pooled features."""
    from randlanet import _hip as H
    torch.manual_seed(d + n)
    K, h = 16, d // 2
    xyz = torch.rand(B, n_parent, 3, device=DEV)
    idx, d2 = ops.knn_i32(xyz, xyz, n, n, K)
    W1, b1 = torch.randn(h, 10, device=DEV) * 0.5, torch.randn(h, device=DEV) * 0.1
    W2, b2 = torch.randn(h, h, device=DEV) / h ** 0.5, torch.randn(h, device=DEV) * 0.1
    g1w, g1b = torch.rand(h, device=DEV) + 0.5, torch.randn(h, device=DEV) * 0.2
    g2w, g2b = torch.rand(h, device=DEV) + 0.5, torch.randn(h, device=DEV) * 0.2
    Gf = torch.randn(B * n_parent, h, device=DEV)
    g = ops.Lazy(Gf, B, n, n_parent, h, torch.rand(h, device=DEV) + 0.5, torch.randn(h, device=DEV) * 0.3, 2, 0.2)
    Ws = torch.randn(d, d, device=DEV) / d ** 0.5
    rows = B * n * K

    def bn(stats, nslots, gamma, beta, c):
        rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
        return ops.bn_finalize(stats, rows, 128, c, gamma, beta, rm, rv, None, 0.99, 1e-6, True, nslots=nslots)

    # stored path
    rpe = ops.rpe_build(ops.Rpe(xyz, idx, d2, B, n, K))
    st1 = ops.new_stats(DEV, h)
    Y1 = ops.gemm(rpe, W1, 1, 10, h, b1, stats=st1)
    s1 = bn(st1, H.row_blocks(rows, 128), g1w, g1b, h)
    u1 = ops.Lazy(Y1, B, n * K, n * K, h, s1[0], s1[1], 1, 0.0, s1[2], s1[3])
    P1 = ops.pool_fwd(u1, g, idx, Ws, n, d)
    st2 = ops.new_stats(DEV, h)
    Y2 = ops.gemm(u1, W2, 1, h, h, b2, stats=st2)
    s2 = bn(st2, H.row_blocks(rows, 128), g2w, g2b, h)
    u2 = ops.Lazy(Y2, B, n * K, n * K, h, s2[0], s2[1], 1, 0.0, s2[2], s2[3])
    P2 = ops.pool_fwd(u2, g, idx, Ws, n, d)
    # virtual path
    vr = ops.VirtualRpe(xyz, idx, d2, B, n, h, W1, b1, W2, b2)
    vs1, ns = ops.rpe_stats(vr, 1)
    t1 = bn(vs1, ns, g1w, g1b, h)
    vr.bn1 = ops.Lazy(d2, B, n * K, n * K, h, t1[0], t1[1], 1, 0.0, t1[2], t1[3])
    V1 = ops.pool_fwd(vr, g, idx, Ws, n, d, stage=1)
    vs2, ns = ops.rpe_stats(vr, 2)
    t2 = bn(vs2, ns, g2w, g2b, h)
    vr.bn2 = ops.Lazy(d2, B, n * K, n * K, h, t2[0], t2[1], 1, 0.0, t2[2], t2[3])
    V2 = ops.pool_fwd(vr, g, idx, Ws, n, d, stage=2)
    tol = 2e-6 if ops.get_wide_gemm() == "fp32" else 5e-5      # the stored path's narrow GEMMs are exact fp32 MFMA chains
    for a, b_, what in ((t1[2], s1[2], "mean1"), (t1[3], s1[3], "invstd1"), (t2[2], s2[2], "mean2"), (t2[3], s2[3], "invstd2")):
        assert float((a - b_).abs().max()) < tol * max(1.0, float(b_.abs().max())), what
    assert float((V1 - P1).abs().max()) < 10 * tol * max(1.0, float(P1.abs().max()))
    assert float((V2 - P2).abs().max()) < 10 * tol * max(1.0, float(P2.abs().max()))
    # the virtual path is a pure function of its inputs: same bits on a second run
    assert torch.equal(V2, ops.pool_fwd(vr, g, idx, Ws, n, d, stage=2))
    # pool1's kernel can leave the stage-2 batch statistics itself (it has the stage-1 tile): same moments as rl_rpe_stats
    V1b, st2b, nsb = ops.pool_fwd(vr, g, idx, Ws, n, d, stage=1, next_stats=True)
    t2b = bn(st2b, nsb, g2w, g2b, h)
    assert torch.equal(V1b, V1)
    assert float((t2b[2] - t2[2]).abs().max()) < 1e-6 * max(1.0, float(t2[2].abs().max()))
    assert float((t2b[3] - t2[3]).abs().max()) < 1e-5 * max(1.0, float(t2[3].abs().max()))
    # round 5: the same statistics as SHIFTED sums around a running mean (rl_pool_desc.pivot_mean*): same moments
    def bn_piv(stats, nslots, gamma, beta, c, rm):
        return ops.bn_finalize(stats, rows, 128, c, gamma, beta, rm.clone(), torch.ones(c, device=DEV), None, 0.99, 1e-6, True,
                               nslots=nslots, pivoted=True)
    vr.piv1 = (t1[2] + 0.05 * torch.randn(h, device=DEV)).contiguous()
    vr.piv2 = (t2[2] + 0.05 * torch.randn(h, device=DEV)).contiguous()
    ps1, ns = ops.rpe_stats(vr, 1)
    p1 = bn_piv(ps1, ns, g1w, g1b, h, vr.piv1)
    ps2, ns = ops.rpe_stats(vr, 2)
    p2 = bn_piv(ps2, ns, g2w, g2b, h, vr.piv2)
    V1c, st2c, nsc = ops.pool_fwd(vr, g, idx, Ws, n, d, stage=1, next_stats=True)
    p2c = bn_piv(st2c, nsc, g2w, g2b, h, vr.piv2)
    assert torch.equal(V1c, V1)
    for a, b_, what in ((p1[2], t1[2], "mean1"), (p1[3], t1[3], "invstd1"), (p2[2], t2[2], "mean2"), (p2[3], t2[3], "invstd2"),
                        (p2c[2], t2[2], "mean2 (pool_fwd)"), (p2c[3], t2[3], "invstd2 (pool_fwd)")):
        assert float((a - b_).abs().max()) < 1e-5 * max(1.0, float(b_.abs().max())), what


@pytest.mark.parametrize("d,B,n_parent,n", [(16, 2, 900, 500), (32, 1, 300, 300), (64, 2, 400, 257), (16, 4, 2048, 2048)])
def test_virtual_rpe_branch_backward(ops, d, B, n_parent, n):
    """rl_pool_bwd with a virtual rpe stage (u_source 1 / 2; its BatchNorm-backward sums) and rl_rpe_wgrad against the same
    block with the mlp_rpe1 / mlp_rpe2 outputs STORED (rl_gemm + the non-virtual rl_pool_bwd + rl_bn_backward + rl_wgrad): the
    gradient of the gathered rows (DG), of the rpe half (GU: added to, and stored), of the score weight, the BatchNorm sums, and
    the weight / bias gradients of both rpe layers."""
    from randlanet import _hip as H
    torch.manual_seed(d + n)
    K, h = 16, d // 2
    xyz = torch.rand(B, n_parent, 3, device=DEV)
    idx, d2 = ops.knn_i32(xyz, xyz, n, n, K)
    W1, b1 = torch.randn(h, 10, device=DEV) * 0.5, torch.randn(h, device=DEV) * 0.1
    W2, b2 = torch.randn(h, h, device=DEV) / h ** 0.5, torch.randn(h, device=DEV) * 0.1
    g1w, g1b = torch.rand(h, device=DEV) + 0.5, torch.randn(h, device=DEV) * 0.2
    g2w, g2b = torch.rand(h, device=DEV) + 0.5, torch.randn(h, device=DEV) * 0.2
    Gf = torch.randn(B * n_parent, h, device=DEV)
    g = ops.Lazy(Gf, B, n, n_parent, h, torch.rand(h, device=DEV) + 0.5, torch.randn(h, device=DEV) * 0.3, 2, 0.2)
    Ws = torch.randn(d, d, device=DEV) / d ** 0.5
    rows, P = B * n * K, B * n
    dP = torch.randn(P, d, device=DEV)

    def bn(stats, nslots, gamma, beta, c):
        rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
        return ops.bn_finalize(stats, rows, 128, c, gamma, beta, rm, rv, None, 0.99, 1e-6, True, nslots=nslots)

    # stored path: Y1 = mlp_rpe1(rpe), Y2 = mlp_rpe2(u1)
    rpe = ops.rpe_build(ops.Rpe(xyz, idx, d2, B, n, K))
    st1 = ops.new_stats(DEV, h)
    Y1 = ops.gemm(rpe, W1, 1, 10, h, b1, stats=st1)
    s1 = bn(st1, H.row_blocks(rows, 128), g1w, g1b, h)
    u1 = ops.Lazy(Y1, B, n * K, n * K, h, s1[0], s1[1], 1, 0.0, s1[2], s1[3])
    st2 = ops.new_stats(DEV, h)
    Y2 = ops.gemm(u1, W2, 1, h, h, b2, stats=st2)
    s2 = bn(st2, H.row_blocks(rows, 128), g2w, g2b, h)
    u2 = ops.Lazy(Y2, B, n * K, n * K, h, s2[0], s2[1], 1, 0.0, s2[2], s2[3])
    # virtual path with the SAME folded BatchNorms
    vr = ops.VirtualRpe(xyz, idx, d2, B, n, h, W1, b1, W2, b2)
    vr.bn1 = ops.Lazy(d2, B, n * K, n * K, h, s1[0], s1[1], 1, 0.0, s1[2], s1[3])
    vr.bn2 = ops.Lazy(d2, B, n * K, n * K, h, s2[0], s2[1], 1, 0.0, s2[2], s2[3])
    tol = 2e-5 if ops.get_wide_gemm() == "fp32" else 2e-4

    def close(a, b_, what, t=tol):
        sc = max(1.0, float(b_.abs().max()))
        assert float((a - b_).abs().max()) < t * sc, (what, float((a - b_).abs().max()), sc)

    for stage, u in ((2, u2), (1, u1)):
        GUs = torch.full((rows, h), 0.25, device=DEV)
        dWs = torch.empty(d, d, device=DEV)
        DGs = ops.pool_bwd(u, g, idx, Ws, n, d, dP, GUs, True, dWs)
        GUv = torch.full((rows, h), 0.25, device=DEV)
        dWv = torch.empty(d, d, device=DEV)
        nslots = H.lib().rl_pool_bwd_slots(P, d)
        bst = torch.empty((nslots, 2, h), dtype=torch.float64, device=DEV)
        DGv = ops.pool_bwd(vr, g, idx, Ws, n, d, dP, GUv, True, dWv, stage=stage, bn_bwd_stats=bst)
        close(DGv, DGs, f"DG stage {stage}")
        close(GUv, GUs, f"GU stage {stage}")
        close(dWv, dWs, f"dW stage {stage}", 10 * tol)
        # the same stage with gu_accumulate off (kernel instantiations of their own on the virtual path): GU is overwritten -
        # a row the launch left alone would stay NaN
        GUs0 = torch.full((rows, h), float("nan"), device=DEV)
        DGs0 = ops.pool_bwd(u, g, idx, Ws, n, d, dP, GUs0, False, torch.empty(d, d, device=DEV))
        GUv0 = torch.full((rows, h), float("nan"), device=DEV)
        DGv0 = ops.pool_bwd(vr, g, idx, Ws, n, d, dP, GUv0, False, torch.empty(d, d, device=DEV), stage=stage)
        close(DGv0, DGs0, f"DG stage {stage}, GU stored")
        close(GUv0, GUs0, f"GU stage {stage}, stored")
        close(GUv0 + 0.25, GUv, f"GU stage {stage}, stored against accumulated")
        # the stage's own backward: BatchNorm sums from the pooling kernel, then the weight / bias / input gradients
        bnl = vr.bn2 if stage == 2 else vr.bn1
        dg_v, db_v = torch.empty(h, device=DEV), torch.empty(h, device=DEV)
        coef = ops.rpe_bn_backward(vr, stage, GUv, dg_v, db_v, stats=bst, nslots=nslots)
        dg_s, db_s = torch.empty(h, device=DEV), torch.empty(h, device=DEV)
        Gs = GUs.clone()
        ops.bn_backward(Gs, u, dg_s, db_s, True)                 # Gs <- gradient w.r.t. the raw stage output
        close(dg_v, dg_s, f"dgamma stage {stage}", 10 * tol)
        close(db_v, db_s, f"dbeta stage {stage}", 10 * tol)
        Kin = 10 if stage == 1 else h
        dWl_v, dbl_v = torch.empty(h, Kin, device=DEV), torch.empty(h, device=DEV)
        pend = []
        GU1 = torch.empty_like(GUv) if stage == 2 else None
        ops.rpe_wgrad(vr, stage, GUv, coef, dWl_v, dbl_v, pend, GU1)
        ops.wgrad_flush(pend)
        dWl_s, dbl_s = torch.empty(h, Kin, device=DEV), torch.empty(h, device=DEV)
        a_in = rpe if stage == 1 else u1
        ops.wgrad(a_in, Gs, n * K, h, dWl_s, 1, Kin, dbl_s)
        close(dWl_v, dWl_s, f"layer dW stage {stage}", 20 * tol)
        # (a bias in front of a BatchNorm: its true gradient is 0 - both sides hold rounding noise of a sum over all rows, and
        # here the virtual side differentiates against the STORED path's batch mean, which differs from the mean of its own
        # recomputed tile by the rounding of a different summation order: a per-row offset of ~1e-7 that the sum multiplies)
        close(dbl_v, dbl_s, f"layer db stage {stage}", max(200 * tol, 3e-6 * rows))
        if stage == 2:
            gl = ops.Lazy(Gs, B, n * K, n * K, h)
            GU1s = torch.empty(rows, h, device=DEV)
            ops.gemm(gl, W2, h, 1, h, None, out=GU1s, out_bstride=n * K)
            # the mask z > 0 of the stage's ReLU is a step: where the two paths' raw values (equal to ~1e-7) straddle 0, a whole
            # row of dY . W2 differs - a handful of the rows x h elements at most
            e1 = (GU1 - GU1s).abs().max(1).values
            sc1 = max(1.0, float(GU1s.abs().max()))
            assert float((e1 > 10 * tol * sc1).float().mean()) < 2e-4, ("GU1", float(e1.max()), sc1)


def test_knn_multi_and_csr_replay_from_a_captured_graph(ops):
    """The neighbour searches of a forward (rl_knn_multi: grid reset, bounding box, counting sort, ring walk) and the
    graph transposes (rl_csr_build) captured into ONE hipGraph and replayed on new coordinates give exactly the eager
    answer - their scratch is reset by kernels of their own (no memset nodes, no allocation inside the region), and the
    per-call workspaces come from the capture's private pool, so their addresses are stable across replays."""
    torch.manual_seed(5)
    B, N = 2, 4096
    xyz = torch.rand(B, N, 3, device=DEV)
    tasks = [(N, N, 16), (N // 4, N // 4, 16), (N // 16, N // 4, 1), (N // 4, N, 1)]

    def run():
        res = ops.knn_multi(xyz, tasks)
        csr = ops.csr_build([(res[i][0], tasks[i][0]) for i in range(len(tasks))])
        return res, csr

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                              # allocator warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res_g, csr_g = run()
    for trial in range(3):
        xyz.copy_(torch.rand(B, N, 3, device=DEV))         # new clouds, same buffers
        g.replay()
        torch.cuda.synchronize()
        res_e, csr_e = run()
        for (ig, dg), (ie, de) in zip(res_g, res_e):
            assert torch.equal(ig, ie) and torch.equal(dg, de), trial
        for a, b in zip(csr_g, csr_e):
            assert torch.equal(a.offsets, b.offsets) and torch.equal(a.entries, b.entries), trial


@pytest.mark.parametrize("M,K,N,orient", [(5000, 256, 256, "fwd"), (3000, 128, 512, "bwd"), (700, 512, 128, "fwd"), (4096, 64, 256, "bwd")])
def test_wide_gemm_with_presplit_weights(ops, request, M, K, N, orient):
    """rl_gemm with W_split (rl_split_weights: bf16 head / tail planes in the product's orientation) runs the 8-wavefront
    kernel; same operands, same MFMA sequence per accumulator -> the SAME BITS as the 4-wavefront kernel, with the lazy
    BatchNorm operand, bias, accumulate, the split epilogue and split-K; statistics agree to rounding."""
    if ops.get_wide_gemm() == "fp32":
        pytest.skip("the pre-split path exists in the bf16 arithmetic modes")
    torch.manual_seed(M + K)
    A = torch.randn(M, K, device=DEV)
    a = ops.plain(A, 1, M)
    a.scale, a.shift, a.act, a.slope = torch.rand(K, device=DEV) + 0.5, torch.randn(K, device=DEV) * 0.3, 2, 0.2
    if orient == "fwd":
        W = torch.randn(N, K, device=DEV) / K ** 0.5            # (out, in): k contiguous
        ks, ns = 1, K
    else:
        W = torch.randn(K, N, device=DEV) / K ** 0.5            # n contiguous: the dgrad orientation
        ks, ns = N, 1
    bias = torch.randn(N, device=DEV)
    ws = ops.split_weights([(W, ks, ns, K, N)])
    assert len(ws) == 1
    st0, st1 = ops.new_stats(DEV, N), ops.new_stats(DEV, N)
    ops.set_gemm_ksplit(False)          # one summation order for both kernels (the LDS-DMA kernel's small tiles split K less often)
    request.addfinalizer(lambda: ops.set_gemm_ksplit(True))
    Y0 = ops.gemm(a, W, ks, ns, N, bias, stats=st0)
    Y1 = ops.gemm(a, W, ks, ns, N, bias, stats=st1, wsplit=ws)
    assert torch.equal(Y0, Y1)
    ref = torch.nn.functional.leaky_relu(A * a.scale + a.shift, 0.2).double() @ (W.double().t() if orient == "fwd" else W.double()) + bias.double()
    assert float((Y1.double() - ref).abs().max()) < 2e-4 * max(1.0, float(ref.abs().max()))
    nsl = ops.gemm_stat_slots(M, N, K)
    assert torch.allclose(st0[:nsl].sum(0), st1[:nsl].sum(0), rtol=2e-6, atol=1e-4)      # per-lane fp32 partial sums, other row grouping
    # accumulate + split epilogue (addend, two destinations)
    acc0 = torch.randn(M, N, device=DEV)
    acc1 = acc0.clone()
    ops.gemm(a, W, ks, ns, N, None, out=acc0, out_bstride=M, accumulate=True)
    ops.gemm(a, W, ks, ns, N, None, out=acc1, out_bstride=M, accumulate=True, wsplit=ws)
    assert torch.equal(acc0, acc1)
    addend = torch.randn(M, N, device=DEV)
    h = N // 2
    o0, o1 = torch.empty(M, h, device=DEV), torch.empty(M, h, device=DEV)
    d0, d1 = torch.empty(M, N - h, device=DEV), torch.empty(M, N - h, device=DEV)
    ops.gemm(a, W, ks, ns, N, None, out=o0, out_bstride=M, addend=addend, out2=d0, split_col=h)
    ops.gemm(a, W, ks, ns, N, None, out=o1, out_bstride=M, addend=addend, out2=d1, split_col=h, wsplit=ws)
    assert torch.equal(o0, o1) and torch.equal(d0, d1)


@pytest.mark.parametrize("M,K,N", [(4099, 128, 192), (2560, 1024, 256), (130, 32, 128), (20480, 256, 256)])
def test_wide_gemm_stagings_agree_bitwise(ops, M, K, N):
    """The two operand stagings of the wide GEMM (rl_set_wgemm_staging: "dma" = wgemm2_kernel, persistent workgroups fed by
    LDS-DMA loader wavefronts, the default; "registers" = wgemm_kernel) run the same products in the same order per
    accumulator: Y is bitwise the same with every epilogue option, rows / columns that do not fill a tile, split-K, a tile
    that straddles split_col; the partial statistics agree after summation (other tiles per slot)."""
    if ops.get_wide_gemm() == "fp32":
        pytest.skip("the pre-split path exists in the bf16 arithmetic modes")
    from randlanet import _hip as H
    torch.manual_seed(M + N)
    A = torch.randn(M, K, device=DEV)
    a = ops.plain(A, 1, M)
    a.scale, a.shift, a.act, a.slope = torch.rand(K, device=DEV) + 0.5, torch.randn(K, device=DEV) * 0.3, 1, 0.0
    W = torch.randn(N, K, device=DEV) / K ** 0.5
    ws = ops.split_weights([(W, 1, K, K, N)])
    bias, addend, old = torch.randn(N, device=DEV), torch.randn(M, N, device=DEV), torch.randn(M, N, device=DEV)
    h = N // 2 if N % 256 == 0 else 96              # 96: the first 128-column tile straddles the split

    def run():
        res = []
        st = ops.new_stats(DEV, N)
        res.append(ops.gemm(a, W, 1, K, N, bias, stats=st, wsplit=ws))
        res.append(st[:ops.gemm_stat_slots(M, N, K)].sum(0))
        acc = old.clone()
        ops.gemm(a, W, 1, K, N, None, out=acc, out_bstride=M, accumulate=True, wsplit=ws)
        res.append(acc)
        o, d = torch.zeros(M, h, device=DEV), torch.zeros(M, N - h, device=DEV)
        ops.gemm(a, W, 1, K, N, None, out=o, out_bstride=M, addend=addend, out2=d, split_col=h, wsplit=ws)
        res += [o, d]
        if M % 4 == 0:                               # Y with a batch stride
            ab = ops.plain(A, 4, M // 4)
            ab.scale, ab.shift, ab.act, ab.slope = a.scale, a.shift, a.act, a.slope
            Yb = torch.zeros(4 * (M // 4 + 5), N, device=DEV)
            ops.gemm(ab, W, 1, K, N, bias, out=Yb, out_bstride=M // 4 + 5, wsplit=ws)
            res.append(Yb)
        torch.cuda.synchronize()
        return res
    try:
        ops.set_gemm_ksplit(False)                   # one summation order on both sides (the LDS-DMA kernel never splits K)
        ops.set_wgemm_staging("registers")
        r0 = run()
        ops.set_wgemm_staging("dma")
        r1 = run()
        ops.set_gemm_ksplit(True)                    # the register-staged kernel as shipped: K split where tiles are few
        ops.set_wgemm_staging("registers")
        r0s = run()
    finally:
        ops.set_wgemm_staging("dma")
        ops.set_gemm_ksplit(True)
    ref = torch.relu(A * a.scale + a.shift).double() @ W.double().t() + bias.double()
    for x, y in zip(r0, r0s):
        assert torch.allclose(x, y, rtol=1e-4, atol=1e-4 * max(1.0, float(ref.abs().max())))
    assert float((r1[0].double() - ref).abs().max()) < 2e-4 * max(1.0, float(ref.abs().max()))
    for i, (x, y) in enumerate(zip(r0, r1)):
        if x.dtype == torch.float64:
            assert torch.allclose(x, y, rtol=1e-12, atol=0.0), i
        else:
            assert torch.equal(x, y), i


@pytest.mark.parametrize("M,K,N", [(5120, 256, 128), (5120, 512, 256), (1280, 512, 512), (5120, 128, 256), (2600, 1024, 192),
                                   (300, 512, 256), (130, 32, 128), (5000, 64, 160), (4099, 256, 100),
                                   (20480, 128, 64), (8192, 256, 32), (3001, 128, 48)])       # (K > 64, N <= 64: 64 x 64 tiles instead of pgemm_kernel)
def test_wide_gemm_tiles_agree_bitwise(ops, M, K, N):
    """The output tile of the LDS-DMA wide GEMM (rl_set_wgemm_tile: "auto" = 64 x 128 / 64 x 64 where 128 x 128 tiles leave most
    CUs without one - the deep levels' launches, round 6; "128" = one tile shape) does not change a product: Y is bitwise the
    same with every epilogue option (bias + statistics, accumulate, addend + two destinations incl. a tile that straddles
    split_col, a batch stride, what is left of split-K), the partial statistics agree after summation (slots per 64 rows)."""
    if ops.get_wide_gemm() == "fp32":
        pytest.skip("the pre-split path exists in the bf16 arithmetic modes")
    torch.manual_seed(M + N + K)
    A = torch.randn(M, K, device=DEV)
    a = ops.plain(A, 1, M)
    a.scale, a.shift, a.act, a.slope = torch.rand(K, device=DEV) + 0.5, torch.randn(K, device=DEV) * 0.3, 2, 0.2
    W = torch.randn(N, K, device=DEV) / K ** 0.5
    Wt = W.t().contiguous()
    ws = ops.split_weights([(W, 1, K, K, N), (Wt, N, 1, K, N)])
    bias, addend, old = torch.randn(N, device=DEV), torch.randn(M, N, device=DEV), torch.randn(M, N, device=DEV)
    piv = torch.randn(N, device=DEV) * 0.1
    h = N // 2 if (N % 256 == 0 or N <= 64) else (96 if N > 128 else 48)

    def run():
        res = []
        st = ops.new_stats(DEV, N)
        res.append(ops.gemm(a, W, 1, K, N, bias, stats=st, wsplit=ws, pivot=(piv, None)))
        res.append(st[:ops.gemm_stat_slots(M, N, K)].sum(0))
        res.append(ops.gemm(a, Wt, N, 1, N, None, wsplit=ws))             # the dgrad orientation, no statistics: transposed accumulator
        acc = old.clone()
        ops.gemm(a, W, 1, K, N, None, out=acc, out_bstride=M, accumulate=True, wsplit=ws)
        res.append(acc)
        if N % 4 == 0:
            o, d = torch.zeros(M, h, device=DEV), torch.zeros(M, N - h, device=DEV)
            ops.gemm(a, W, 1, K, N, None, out=o, out_bstride=M, addend=addend, out2=d, split_col=h, wsplit=ws)
            res += [o, d]
        if M % 4 == 0:
            ab = ops.plain(A, 4, M // 4)
            ab.scale, ab.shift, ab.act, ab.slope = a.scale, a.shift, a.act, a.slope
            Yb = torch.zeros(4 * (M // 4 + 5), N, device=DEV)
            ops.gemm(ab, W, 1, K, N, bias, out=Yb, out_bstride=M // 4 + 5, wsplit=ws)
            res.append(Yb)
        torch.cuda.synchronize()
        return res
    try:
        ops.set_gemm_ksplit(False)
        ops.set_wgemm_tile("128")
        r0 = run()
        ops.set_wgemm_tile("auto")
        r1 = run()
        ops.set_gemm_ksplit(True)                    # as shipped (the switch does not reach the LDS-DMA kernel: it never splits K)
        r2 = run()
    finally:
        ops.set_wgemm_tile("auto")
        ops.set_gemm_ksplit(True)
    ref = torch.nn.functional.leaky_relu(A * a.scale + a.shift, 0.2).double() @ W.double().t() + bias.double()
    assert float((r1[0].double() - ref).abs().max()) < 2e-4 * max(1.0, float(ref.abs().max()))
    assert float((r2[0].double() - ref).abs().max()) < 2e-4 * max(1.0, float(ref.abs().max()))
    for x, y in zip(r1, r2):
        assert torch.allclose(x, y, rtol=1e-4, atol=1e-4 * max(1.0, float(ref.abs().max())))
    for i, (x, y) in enumerate(zip(r0, r1)):
        if x.dtype == torch.float64:
            assert torch.allclose(x, y, rtol=1e-6, atol=1e-3), i       # (fp32 per-lane partial sums over another set of rows)
        else:
            assert torch.equal(x, y), i


@pytest.mark.parametrize("M,K,N1,N2,stats", [(10240, 128, 32, 128, True), (2560, 128, 64, 256, True), (1300, 256, 128, 512, True),
                                             (4099, 96, 32, 100, False), (640, 256, 128, 512, False)])
def test_gemm_pair_equals_two_launches(ops, M, K, N1, N2, stats):
    """rl_gemm_pair (mlp1 + shortcut of an encoder level in one launch of the LDS-DMA wide GEMM, round 6): both outputs bitwise
    what two rl_gemm calls give on the same 128 x 128 tiles, the partial statistics of each product in its own buffer (equal
    after summation), lazy operand, pivots, rows / columns that do not fill a tile."""
    if ops.get_wide_gemm() == "fp32":
        pytest.skip("the pre-split path exists in the bf16 arithmetic modes")
    from randlanet import _hip as H
    torch.manual_seed(M + N1)
    A = torch.randn(2 * M + 7, K, device=DEV)[:2 * M]
    a = ops.plain(A, 2, M)
    a.scale, a.shift, a.act, a.slope = torch.rand(K, device=DEV) + 0.5, torch.randn(K, device=DEV) * 0.3, 2, 0.2
    W1, W2 = torch.randn(N1, K, device=DEV) / K ** 0.5, torch.randn(N2, K, device=DEV) / K ** 0.5
    p1, p2 = torch.randn(N1, device=DEV) * 0.1, torch.randn(N2, device=DEV) * 0.1
    b2 = torch.randn(N2, device=DEV) * 0.1
    ws = ops.split_weights([(W1, 1, K, K, N1, True), (W2, 1, K, K, N2)])
    assert len(ws) == 2
    nsl = H.row_blocks(2 * M, 128)
    try:
        ops.set_wgemm_tile("128")                       # the pair runs on 128 x 128 tiles: the same slots and sums ...
        ops.set_gemm_ksplit(False)                      # ... in one pass over K ("128" alone restores round 5's K splits too)
        ref, st = [], []
        for W, N, piv in ((W1, N1, (p1, None)), (W2, N2, (p2, b2))):
            s = ops.new_stats(DEV, N) if stats else None
            ref.append(ops.gemm(a, W, 1, K, N, None, stats=s, wsplit=ws, pivot=piv if stats else None))
            st.append(s)
    finally:
        ops.set_wgemm_tile("auto")
        ops.set_gemm_ksplit(True)
    s1, s2 = (ops.new_stats(DEV, N1), ops.new_stats(DEV, N2)) if stats else (None, None)
    res = ops.gemm_pair(a, (W1, 1, K, N1, s1, (p1, None) if stats else None), (W2, 1, K, N2, s2, (p2, b2) if stats else None), ws)
    assert res is not None, "rl_gemm_pair refused a pair it should take"
    assert H.lib().rl_last_kernel().decode() == "wgemm2_kernel"
    torch.cuda.synchronize()
    assert torch.equal(res[1], ref[1])
    assert torch.equal(res[0], ref[0])      # (K > 64: the narrow product alone runs on the LDS-tiled kernel, the same arithmetic)
    if stats:
        if N1 > 64:
            assert torch.allclose(s1[:nsl].sum(0), st[0][:nsl].sum(0), rtol=1e-12, atol=0.0)
        assert torch.allclose(s2[:nsl].sum(0), st[1][:nsl].sum(0), rtol=1e-12, atol=0.0)
    fp64 = torch.nn.functional.leaky_relu(A * a.scale + a.shift, 0.2).double()
    for Y, W in zip(res, (W1, W2)):
        r = fp64 @ W.double().t()
        assert float((Y.double() - r).abs().max()) < 2e-4 * max(1.0, float(r.abs().max()))
    if stats:       # the narrow product's statistics against the result itself (shifted sums around its pivot)
        d = res[0].double() - p1.double()
        assert torch.allclose(s1[:nsl, 0].sum(0), d.sum(0), rtol=1e-5, atol=1e-3)
        assert torch.allclose(s1[:nsl, 1].sum(0), (d * d).sum(0), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("M,K,N,act,accumulate", [(5000, 32, 64, 1, False), (4099, 64, 8, 2, False), (3000, 8, 8, 2, True), (2600, 32, 16, 0, False)])
def test_streaming_gemm_leaves_bn_backward_sums(ops, M, K, N, act, accumulate):
    """rl_gemm_desc.bnb_* (round 6): an input-gradient product on the streaming kernel that completes the gradient of a BatchNorm
    layer's output also leaves that layer's BatchNorm-backward sums - G bitwise what the plain product gives, the sums those of
    rl_bn_bwd_reduce over the same G and Y, and the whole backward (dgamma, dbeta, dY) equal to the three-launch form."""
    import ctypes
    from randlanet import _hip as H
    torch.manual_seed(M + K)
    dY = torch.randn(M, K, device=DEV)
    W = torch.randn(K, N, device=DEV) / K ** 0.5                      # (in, out) of the layer BEHIND: dA = dY . W, n contiguous
    Yl = torch.randn(M, N, device=DEV)
    mean, var = Yl.mean(0), Yl.var(0, unbiased=False)
    gamma, beta = torch.rand(N, device=DEV) + 0.5, torch.randn(N, device=DEV) * 0.2
    invstd = torch.rsqrt(var + 1e-6)
    scale = gamma * invstd
    y = ops.Lazy(Yl, 1, M, M, N, scale, beta - mean * scale, act, 0.2 if act == 2 else 0.0, mean, invstd, "x")
    old = torch.randn(M, N, device=DEV)
    a = ops.plain(dY, 1, M)

    def product(bnb):
        out = old.clone() if accumulate else torch.empty(M, N, device=DEV)
        return ops.gemm(a, W, N, 1, N, None, out=out, out_bstride=M, accumulate=accumulate, bnb=bnb)
    G0 = product(None)
    G1, pre = product(y)
    assert pre is not None, "the streaming kernel should have taken this product"
    assert H.lib().rl_last_kernel().decode() == "sgemm_kernel"
    assert torch.equal(G0, G1)
    # the sums of rl_bn_bwd_reduce over the same G and Y
    st = ops.new_stats(DEV, N)
    d = ops._bn_bwd_desc(G0, M, y)
    d.stats = st.data_ptr()
    H.check(H.lib().rl_bn_bwd_reduce(ctypes.byref(d), ops._st()), "rl_bn_bwd_reduce")
    ref = st[:H.lib().rl_bn_bwd_slots(M)].sum(0)
    got = pre[0][:pre[1]].sum(0)
    scale_s = float(ref.abs().max()) + 1e-6
    assert float((got - ref).abs().max()) < 2e-5 * scale_s + 1e-4, (got, ref)
    # ... and the backward they drive
    res = []
    for stats in (None, pre):
        G = G0.clone()
        dg, db = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
        ops.bn_backward(G, y, dg, db, True, stats=stats)
        res.append((G, dg, db))
    for u, v in zip(*res):
        assert torch.allclose(u, v, rtol=1e-4, atol=1e-5 * max(1.0, float(v.abs().max())))


def test_gemm_pair_leaves_exact_fp32_products_alone(ops):
    """A product with K <= 64 and N <= 64 runs on the streaming kernel in exact fp32 products: rl_gemm_pair does not take it (its
    arithmetic would become bf16x3) - the caller issues two launches."""
    if ops.get_wide_gemm() == "fp32":
        pytest.skip("the pre-split path exists in the bf16 arithmetic modes")
    M, K, N1, N2 = 2048, 32, 32, 128
    A = torch.randn(M, K, device=DEV)
    W1, W2 = torch.randn(N1, K, device=DEV), torch.randn(N2, K, device=DEV)
    ws = ops.split_weights([(W1, 1, K, K, N1, True), (W2, 1, K, K, N2)])
    assert ops.gemm_pair(ops.plain(A, 1, M), (W1, 1, K, N1, None, None), (W2, 1, K, N2, None, None), ws) is None


def test_wide_gemm_dispatch_names_the_kernel_it_ran(ops):
    """rl_last_kernel after rl_gemm: the LDS-DMA kernel by default where it applies (K % 32 == 0, K <= 1024, pre-split weights),
    the register-staged one on request and for K % 32 != 0, the 4-wavefront kernel without planes, the streaming kernel for
    narrow layers - so a silent fallback to a slower path shows up in a test, not in a profile.  Also the split-K launches, the
    split-scatter epilogue (addend) and the fp32 arithmetic mode."""
    from randlanet import _hip as H
    last = lambda: H.lib().rl_last_kernel().decode()
    mode0 = ops.get_wide_gemm()
    B3, F = "bf16x3", "fp32"
    for M, K, N, planes, staging, want, mode, tile, split in [
            (20000, 256, 128, True, "dma", "wgemm2_kernel", B3, "auto", False), (20000, 256, 128, True, "registers", "wgemm_kernel", B3, "auto", False),
            (20000, 40, 128, True, "dma", "wgemm_kernel", B3, "auto", False), (20000, 256, 128, False, "dma", "pgemm_kernel<8>", B3, "auto", False),
            (3000, 512, 256, True, "dma", "wgemm2_kernel", B3, "auto", False),        # (64 x 64 tiles: 188 of them, no K split)
            (300, 512, 256, True, "dma", "wgemm2_kernel", B3, "auto", False),         # (the LDS-DMA kernel never splits K)
            (20000, 256, 64, True, "dma", "wgemm2_kernel", B3, "auto", False), (20000, 256, 64, False, "dma", "pgemm_kernel<4>", B3, "auto", False),
            (300, 512, 256, True, "registers", "wgemm_kernel+splitk", B3, "auto", False), (3000, 64, 64, False, "dma", "sgemm_kernel", B3, "auto", False),
            # split K: the 128 x 128 tiles of rl_set_wgemm_tile("128") split K on the LDS-DMA kernel too; without planes pgemm_kernel<8>
            (300, 512, 256, True, "dma", "wgemm2_kernel+splitk", B3, "128", False), (300, 512, 256, False, "dma", "pgemm_kernel<8>+splitk", B3, "auto", False),
            (20000, 256, 16, False, "dma", "pgemm_kernel<1>", B3, "auto", False), (20000, 256, 32, False, "dma", "pgemm_kernel<2>", B3, "auto", False),
            (20000, 10, 128, False, "dma", "gemm_kernel", B3, "auto", False),       # (K % 4 != 0: no 16-byte loads)
            # the split-scatter epilogue (addend): pgemm / wgemm only, never split K
            (20000, 256, 64, False, "dma", "pgemm_kernel", B3, "auto", True), (20000, 256, 128, False, "dma", "pgemm_kernel<8>", B3, "auto", True),
            (20000, 256, 128, True, "dma", "wgemm2_kernel", B3, "auto", True), (300, 512, 256, True, "registers", "wgemm_kernel", B3, "auto", True),
            # fp32 arithmetic: no pre-split planes
            (20000, 256, 128, True, "dma", "pgemm_kernel<8>", F, "auto", False), (300, 512, 256, True, "dma", "pgemm_kernel<8>+splitk", F, "auto", False),
            (20000, 256, 128, True, "dma", "pgemm_kernel<8>", F, "auto", True)]:
        A = torch.randn(M, K, device=DEV)
        W = torch.randn(N, K, device=DEV)
        try:
            ops.set_wide_gemm(mode)
            ops.set_wgemm_staging(staging)
            ops.set_wgemm_tile(tile)
            ws = ops.split_weights([(W, 1, K, K, N)]) if planes else None
            addend = torch.randn(M, N, device=DEV) if split else None
            ops.gemm(ops.plain(A, 1, M), W, 1, K, N, wsplit=ws, addend=addend)
            assert last() == want, (M, K, N, planes, staging, mode, tile, split, last())
        finally:
            ops.set_wide_gemm(mode0)
            ops.set_wgemm_staging("dma")
            ops.set_wgemm_tile("auto")


def test_weight_gradient_dispatch_names_the_kernel_it_ran(ops):
    """rl_last_kernel after rl_wgrad / rl_wgrad_batch: every kernel the weight gradient can run, by shape, alignment, row type
    and arithmetic mode."""
    from randlanet import _hip as H
    last = lambda: H.lib().rl_last_kernel().decode()
    mode0 = ops.get_wide_gemm()
    B3, F = "bf16x3", "fp32"
    for M, K, N, mode, bf16, batched, want in [
            (5000, 32, 32, B3, False, False, "swgrad_kernel"), (5000, 16, 128, B3, False, False, "swgrad_kernel"),
            (5000, 256, 128, B3, False, False, "pwgrad128w_kernel"), (5000, 256, 128, "bf16", False, False, "pwgrad128w_kernel"),
            (5000, 256, 128, F, False, False, "pwgrad128_kernel"), (5000, 256, 128, B3, True, False, "pwgrad128w_kernel"),
            (5000, 96, 96, B3, False, False, "pwgrad_kernel"), (5000, 90, 96, B3, False, False, "wgrad_kernel"),
            (5000, 256, 128, B3, False, True, "pwgrad128w_batch_kernel"), (5000, 32, 32, B3, False, True, "swgrad_batch_kernel")]:
        dt = torch.bfloat16 if bf16 else torch.float32
        A = torch.randn(M, K, device=DEV).to(dt)
        dY = torch.randn(M, N, device=DEV).to(dt)
        dW, db = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
        try:
            ops.set_wide_gemm(mode)
            pending, batch = ([], []) if batched else (None, None)
            ops.wgrad(ops.plain(A, 1, M), dY, M, N, dW, 1, K, db, pending=pending, batch=batch)
            if batched:
                assert len(batch) == 1, (M, K, N)
                ops.wgrad_batch_flush(batch)
            assert last() == want, (M, K, N, mode, bf16, batched, last())
            if batched:
                ops.wgrad_flush(pending)
        finally:
            ops.set_wide_gemm(mode0)


def test_float_atomic_entry_points_need_an_opt_in(ops, monkeypatch):
    """rl_scatter_add_rows / rl_gemm(out2_index) add with fp32 atomics: not part of the schedule, refused by default."""
    monkeypatch.delenv("RL_ALLOW_FLOAT_ATOMICS", raising=False)
    src = torch.ones(8, 4, device=DEV)
    dst = torch.zeros(4, 4, device=DEV)
    idx = torch.zeros(8, dtype=torch.int32, device=DEV)
    with pytest.raises(Exception, match="RL_ALLOW_FLOAT_ATOMICS"):
        ops.scatter_add_rows(src, (0, 4), dst, 4, 8, 8, idx)
    assert float(dst.abs().sum()) == 0.0


def test_grouped_wide_weight_gradients_equal_the_single_launches_bitwise(ops):
    """rl_wgrad_batch: several layers' weight gradients as ONE launch per kind (wide 128 x 128-tile kernel / narrow streaming
    kernel, every (KT, NT) body of it) - same split, same per-workgroup arithmetic, so the same bits as one rl_wgrad launch
    per layer."""
    torch.manual_seed(5)
    shapes = [(5000, 128, 256, False), (2000, 256, 128, True), (700, 512, 256, False), (9000, 96, 160, False), (3000, 32, 32, False),
              (7001, 8, 8, True), (4000, 16, 32, False), (3333, 8, 64, True), (2500, 10, 128, False), (6000, 32, 16, True),
              (5000, 24, 64, False), (4100, 64, 8, True), (3900, 64, 32, False), (8000, 64, 64, True), (100, 48, 40, False)]
    layers = []
    for M, K, N, lazy in shapes:
        A = torch.randn(M, K, device=DEV)
        dY = torch.randn(M, N, device=DEV)
        a = ops.Lazy(A, 1, M, M, K, torch.rand(K, device=DEV) + 0.5, torch.randn(K, device=DEV) * 0.1, 2, 0.2) if lazy else ops.plain(A, 1, M)
        layers.append((a, dY, M, K, N))

    def run(batched):
        outs, pending, batch = [], [], ([] if batched else None)
        for a, dY, M, K, N in layers:
            dW, db = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
            ops.wgrad(a, dY, M, N, dW, 1, K, db, pending=pending, batch=batch)
            outs.append((dW, db))
        queued = len(batch) if batched else 0
        if batched:
            ops.wgrad_batch_flush(batch)
        ops.wgrad_flush(pending)
        torch.cuda.synchronize()
        return outs, queued
    single, _ = run(False)
    grouped, queued = run(True)
    assert queued == len(layers)                         # four wide layers, eleven narrow ones: two grouped launches
    for (w0, b0), (w1, b1), (a, dY, M, K, N) in zip(single, grouped, layers):
        assert torch.equal(w0, w1) and torch.equal(b0, b1), (M, K, N)
    a, dY, M, K, N = layers[0]
    ref = dY.double().t() @ a.raw.double()
    assert float((grouped[0][0].double() - ref).abs().max()) < 1e-3 * float(ref.abs().max())
    # more layers than one launch's table holds (24): the entry point chunks
    layers = [(ops.plain(torch.randn(300 + 7 * i, 128, device=DEV), 1, 300 + 7 * i), torch.randn(300 + 7 * i, 128, device=DEV), 300 + 7 * i, 128, 128)
              for i in range(27)]
    single, _ = run(False)
    grouped, queued = run(True)
    assert queued == 27
    assert all(torch.equal(w0, w1) and torch.equal(b0, b1) for (w0, b0), (w1, b1) in zip(single, grouped))


def _morton4(c):
    code = np.zeros(len(c), dtype=np.int64)
    for a in range(3):
        for bit in range(4):
            code |= ((c[:, a] >> bit) & 1) << (3 * bit + a)
    return code


@pytest.mark.parametrize("B,N,cin,edges", [
    (3, 5000, 5, [0, 19, 78, 312, 1250, 5000]),
    (8, 40960, 3, [0, 160, 640, 2560, 10240, 40960]),        # the metric's shape
    (2, 1031, 4, [0, 257, 1031]),                            # two bands, ragged tiles
])
def test_band_sort_is_a_stable_cell_sort_inside_the_bands(ops, B, N, cin, edges):
    """rl_band_sort against its definition: per cloud, every band of the permutation ordered by the 4096-cell Morton code of
    the cloud's points, ties in the permutation's own order (a STABLE sort: deterministic), nothing moved across a band edge."""
    rs = np.random.RandomState(B * 7 + N)
    x = rs.normal(0, 1, (B, N, cin)).astype(np.float32)
    x[0, :, 1] = 0.25                                        # a cloud that is flat in y: extent 0 on one axis
    perm = rs.permutation(N).astype(np.int64)
    out = ops.band_sort(torch.from_numpy(x).to(DEV), torch.from_numpy(perm).to(DEV), edges).cpu().numpy()
    out2 = ops.band_sort(torch.from_numpy(x).to(DEV), torch.from_numpy(perm).to(DEV), edges).cpu().numpy()
    assert np.array_equal(out, out2)                         # (no arrival order in it)
    for b in range(B):
        xyz = x[b, :, :3]
        lo, hi = xyz.min(0), xyz.max(0)
        ext = (hi - lo).astype(np.float32)
        sc = np.where(ext > 0, np.float32(16.0) / np.where(ext > 0, ext, 1), 0).astype(np.float32)
        cells = np.clip(((xyz - lo).astype(np.float32) * sc).astype(np.int64), 0, 15)
        code = _morton4(cells)
        want = perm.copy()
        for a, e in zip(edges[:-1], edges[1:]):
            seg = perm[a:e]
            want[a:e] = seg[np.argsort(code[seg], kind="stable")]
        assert np.array_equal(out[b], want), (b, int((out[b] != want).sum()))
