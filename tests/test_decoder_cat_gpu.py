"""A decoder step without a stored concat: [act(bn(x))[nn] | skip] read in place, the gathered half first.

Library level: rl_gemm / rl_wgrad / rl_wgrad_batch with the operand (rl_*_desc.a2_* with a2_first = 1: x, nn, skip) against
rl_copy_rows_pair into a stored concat followed by the same entry point on it - Y, the statistics slots, the partial slabs and
their bias sums are compared as bytes (torch.equal); nothing has a tolerance.  The wide kernels (wgemm2_cat_kernel,
pwgrad128w_body) and the streaming ones (the sgemm / swgrad concat-gather instantiations), a grouped launch with six concat
layers of both column orders, and the streaming kernel's dense split store (out2 / split_col) against one store plus
rl_copy_rows of the right half.  Engine level: TrainStep "in_place" against "stored" with the row bound at 0.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _sources(B, n_f, n_c, C1, C2, seed):
    """x: the coarse level's output as a per-point table with BatchNorm + ReLU, a prefix view (batch stride n_c + 3 > n_c) of
    wider rows (C1 + 8); skip: dense rows without a fold; nn (B, n_f, 1) with 0, n_c - 1 and repeated indices."""
    from randlanet import _hip as H
    from randlanet import _ops as ops
    g = torch.Generator().manual_seed(seed)
    to = lambda t: t.to(DEV).contiguous()
    xb = n_c + 3
    x_raw = torch.randn((B * xb, C1 + 8), generator=g)
    s_raw = torch.randn((B * n_f, C2), generator=g)
    sc, sh = torch.empty(C1).uniform_(-1.5, 1.5, generator=g), torch.empty(C1).uniform_(-0.5, 0.5, generator=g)
    nn = torch.randint(0, n_c, (B, n_f, 1), generator=g, dtype=torch.int32)
    nn[:, 0] = 0
    nn[:, 1] = n_c - 1
    nn[:, 3] = nn[:, 2]
    nn[:, 5] = nn[:, 2]
    nn[:, n_f - 1] = 0
    nn[:, n_f - 2] = n_c - 1
    x = ops.Lazy(to(x_raw), B, n_c, xb, C1, to(sc), to(sh), H.ACT_RELU, 0.0)
    skip = ops.Lazy(to(s_raw), B, n_f, n_f, C2)
    return x, skip, to(nn)


def _stored(x, skip, nn, first=True):
    """The concat as the engine's stored path builds it (first: [x[nn] | skip], else [skip | x[nn]])."""
    from randlanet import _ops as ops
    rows, n_f = skip.rows, skip.n
    cat = torch.empty((rows, x.C + skip.C), dtype=torch.float32, device=DEV)
    c_x, c_s = (0, x.C) if first else (skip.C, 0)
    ops.copy_rows_pair(((x.raw, (0, x.C), x.bstride, cat, (c_x, x.C), rows, n_f), dict(index=nn, lazy=x)),
                       ((skip.raw, (0, skip.C), skip.bstride, cat, (c_s, skip.C), rows, n_f), {}))
    return cat


def _reference(x, skip, nn):
    xv = x.raw.view(x.B, x.bstride, -1)[:, :, :x.C]
    rows = torch.stack([xv[b][nn[b].reshape(-1).long()] for b in range(x.B)]).reshape(-1, x.C)
    return torch.cat([torch.relu(rows * x.scale + x.shift), skip.raw], dim=1)


def _weights(K, N, seed):
    from randlanet import _ops as ops
    W = (torch.randn((N, K), generator=torch.Generator().manual_seed(seed)) * 0.1).to(DEV)
    return W, ops.split_weights([(W, 1, K, K, N)])


# B, n_f, n_c, C1 = C2, N
WIDE = {
    "a 64-row tile spans two clouds, ragged last tile": (2, 48, 12, 128, 32),
    "64 x 128 and 128 x 128 tiles": (3, 80, 20, 256, 128),
    "K = 1024": (2, 16, 4, 512, 256),
}
STREAM = {"two clouds": (2, 48, 12, 32, 8), "rows per cloud no multiple of 16": (3, 1000, 250, 32, 8)}


@pytest.fixture(scope="module")
def cases():
    out = {}
    for i, (name, (B, n_f, n_c, C, N)) in enumerate({**WIDE, **STREAM}.items()):
        x, skip, nn = _sources(B, n_f, n_c, C, C, 100 + i)
        cat = _stored(x, skip, nn)
        W, planes = _weights(2 * C, N, 200 + i)
        dY = torch.randn((B * n_f, N), generator=torch.Generator().manual_seed(300 + i)).to(DEV)
        out[name] = dict(B=B, n_f=n_f, C=C, N=N, x=x, skip=skip, nn=nn, cat=cat, W=W, planes=planes, dY=dY)
    torch.cuda.synchronize()
    return out


@pytest.fixture()
def settings():
    from randlanet import _ops as ops
    mode0 = ops.get_wide_gemm()
    yield ops
    ops.set_wide_gemm(mode0)


def test_stored_concat_is_the_reference(cases):
    for name, k in cases.items():
        assert torch.equal(k["cat"], _reference(k["x"], k["skip"], k["nn"])), name
        assert float((k["cat"][:, :k["C"]] == 0).float().mean()) > 0.2, name


@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("case", sorted(WIDE))
def test_wide_product_from_the_two_sources(cases, settings, case, mode, stats):
    from randlanet import _hip as H
    ops = settings
    k = cases[case]
    B, n_f, N, W, cat = k["B"], k["n_f"], k["N"], k["W"], k["cat"]
    K, M = 2 * k["C"], cat.shape[0]
    ops.set_wide_gemm(mode)
    a = ops.InterpConcat(k["x"], k["skip"], k["nn"])
    assert ops.gemm_concat_supported(a, W, 1, K, N, k["planes"])
    slots = ops.gemm_stat_slots(M, N, K)
    st_s = ops.new_stats(DEV, N).fill_(-1.0) if stats else None
    st_t = ops.new_stats(DEV, N).fill_(-2.0) if stats else None
    Ys = ops.gemm(ops.plain(cat, B, n_f), W, 1, K, N, None, wsplit=k["planes"], stats=st_s)
    assert H.lib().rl_last_kernel() == b"wgemm2_kernel"
    Yt = ops.gemm(a, W, 1, K, N, None, wsplit=k["planes"], stats=st_t)
    assert H.lib().rl_last_kernel() == b"wgemm2_kernel<cat>"
    torch.cuda.synchronize()
    ref = cat.double() @ W.double().t()
    print(f"{case} {mode}: M {M} K {K} N {N}, error against fp64: stored {float((Ys.double() - ref).abs().max()):.3e}, "
          f"two sources {float((Yt.double() - ref).abs().max()):.3e}")
    assert torch.isfinite(Yt).all() and float(Yt.abs().max()) > 0
    assert torch.equal(Yt.view(torch.int32), Ys.view(torch.int32))
    if stats:
        assert torch.equal(st_t[:slots].view(torch.int64), st_s[:slots].view(torch.int64))
        assert bool((st_t[slots:] == -2.0).all()), "slots beyond rl_gemm_stat_slots were written"


def _slabs(ops, a, dY, n_f, N, K, grouped):
    """The partial slabs (with their bias sums) of rl_wgrad, or of the layer inside a grouped launch; and dW, dbias."""
    from randlanet import _hip as H
    M = dY.shape[0]
    nsplit, per = H.lib().rl_wgrad_nsplit(M, N, K), N * K + N
    dW, db = torch.zeros(N * K, device=DEV), torch.zeros(N, device=DEV)
    if not grouped:
        ops.wgrad(a, dY, n_f, N, dW, 1, K, db)
        name = H.lib().rl_last_kernel()
        slab = ops._slab(DEV, nsplit * per)[:nsplit * per].clone()
    else:
        pending, batch = [], []
        ops.wgrad(a, dY, n_f, N, dW, 1, K, db, pending=pending, batch=batch)
        assert len(batch) == 1, "the layer must join the grouped launch"
        ops.wgrad_batch_flush(batch)
        name = H.lib().rl_last_kernel()
        slab = pending[0][1][:nsplit * per].clone()
        ops.wgrad_flush(pending)
    return slab, dW, db, name


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("case", sorted(WIDE))
def test_wide_weight_gradient_from_the_two_sources(cases, settings, case, mode):
    ops = settings
    k = cases[case]
    B, n_f, N, cat, dY = k["B"], k["n_f"], k["N"], k["cat"], k["dY"]
    K = 2 * k["C"]
    ops.set_wide_gemm(mode)
    a = ops.InterpConcat(k["x"], k["skip"], k["nn"])
    assert ops.wgrad_supported(a, dY, n_f, N)
    for grouped in (False, True):
        slab_s, dW_s, db_s, name_s = _slabs(ops, ops.plain(cat, B, n_f), dY, n_f, N, K, grouped)
        slab_t, dW_t, db_t, name_t = _slabs(ops, a, dY, n_f, N, K, grouped)
        torch.cuda.synchronize()
        assert name_t == name_s == (b"pwgrad128w_batch_kernel" if grouped else b"pwgrad128w_kernel")
        assert float(slab_t.abs().max()) > 0
        assert torch.equal(slab_t.view(torch.int32), slab_s.view(torch.int32)), grouped
        assert torch.equal(dW_t, dW_s) and torch.equal(db_t, db_s), grouped


def test_grouped_launch_with_six_concat_layers_of_both_orders(cases, settings):
    """More second sources than the four a grouped launch used to carry, [gathered | direct] and [direct | gathered] mixed, in
    ONE launch: every layer's slab is that of its own rl_wgrad launch, and of the stored concat's."""
    from randlanet import _hip as H
    ops = settings
    ops.set_wide_gemm("bf16x3")
    layers = []
    for name in sorted(WIDE):
        k = cases[name]
        for first in (True, False):
            a = ops.InterpConcat(k["x"], k["skip"], k["nn"]) if first else ops.ConcatGather(k["skip"], k["x"], k["nn"])
            cat = k["cat"] if first else _stored(k["x"], k["skip"], k["nn"], first=False)
            layers.append((a, cat, k))
    assert len(layers) == 6
    single, stored = [], []
    for a, cat, k in layers:
        single.append(_slabs(ops, a, k["dY"], k["n_f"], k["N"], 2 * k["C"], False)[0])
        stored.append(_slabs(ops, ops.plain(cat, k["B"], k["n_f"]), k["dY"], k["n_f"], k["N"], 2 * k["C"], False)[0])
    pending, batch, outs = [], [], []
    for a, cat, k in layers:
        N, K = k["N"], 2 * k["C"]
        dW, db = torch.zeros(N * K, device=DEV), torch.zeros(N, device=DEV)
        ops.wgrad(a, k["dY"], k["n_f"], N, dW, 1, K, db, pending=pending, batch=batch)
        outs.append((dW, db))
    assert len(batch) == 6 and all(b[6] == 1 for b in batch)
    launches = H.lib().rl_launch_count()
    ops.wgrad_batch_flush(batch)
    assert H.lib().rl_launch_count() == launches + 1, "six concat-gather layers must fit one grouped launch"
    torch.cuda.synchronize()
    for i, ((a, cat, k), p) in enumerate(zip(layers, pending)):
        N, K = k["N"], 2 * k["C"]
        used = H.lib().rl_wgrad_nsplit(cat.shape[0], N, K) * (N * K + N)
        got = p[1][:used]
        assert torch.equal(got.view(torch.int32), single[i].view(torch.int32)), i
        assert torch.equal(got.view(torch.int32), stored[i].view(torch.int32)), i
    ops.wgrad_flush(pending)


@pytest.mark.parametrize("case", sorted(STREAM))
def test_streaming_product_and_weight_gradient_from_the_two_sources(cases, settings, case):
    from randlanet import _hip as H
    ops = settings
    k = cases[case]
    B, n_f, N, W, cat, dY = k["B"], k["n_f"], k["N"], k["W"], k["cat"], k["dY"]
    K, M = 2 * k["C"], cat.shape[0]
    assert (K, N) == (64, 8)
    a = ops.InterpConcat(k["x"], k["skip"], k["nn"])
    if not ops.gemm_concat_supported(a, W, 1, K, N, None):
        # (the plan refuses the shape: the refusal code, and nothing launched)
        launches = H.lib().rl_launch_count()
        with pytest.raises(H.HipKernelError):
            ops.gemm(a, W, 1, K, N, None)
        assert H.lib().rl_launch_count() == launches and not ops.wgrad_supported(a, dY, n_f, N)
        return
    slots = ops.gemm_stat_slots(M, N, K)
    st_s, st_t = ops.new_stats(DEV, N).fill_(-1.0), ops.new_stats(DEV, N).fill_(-2.0)
    Ys = ops.gemm(ops.plain(cat, B, n_f), W, 1, K, N, None, stats=st_s)
    assert H.lib().rl_last_kernel() == b"sgemm_kernel"
    Yt = ops.gemm(a, W, 1, K, N, None, stats=st_t)
    assert H.lib().rl_last_kernel() == b"sgemm_kernel<cat>"
    torch.cuda.synchronize()
    assert float(Yt.abs().max()) > 0
    assert torch.equal(Yt.view(torch.int32), Ys.view(torch.int32))
    assert torch.equal(st_t[:slots].view(torch.int64), st_s[:slots].view(torch.int64))
    assert bool((st_t[slots:] == -2.0).all()), "slots beyond rl_gemm_stat_slots were written"
    # the weight gradient: alone, and queued for the grouped launch of the narrow layers
    assert ops.wgrad_supported(a, dY, n_f, N)
    for grouped in (False, True):
        slab_s, dW_s, db_s, name_s = _slabs(ops, ops.plain(cat, B, n_f), dY, n_f, N, K, grouped)
        slab_t, dW_t, db_t, name_t = _slabs(ops, a, dY, n_f, N, K, grouped)
        torch.cuda.synchronize()
        assert name_s == (b"swgrad_batch_kernel" if grouped else b"swgrad_kernel")
        assert name_t == (b"swgrad_batch_kernel" if grouped else b"swgrad_kernel<cat>")
        assert float(slab_t.abs().max()) > 0
        assert torch.equal(slab_t.view(torch.int32), slab_s.view(torch.int32)), grouped
        assert torch.equal(dW_t, dW_s) and torch.equal(db_t, db_s), grouped


@pytest.mark.parametrize("M", [40, 4096])
def test_streaming_split_store(settings, M):
    """K = 8 -> N = 64, split_col = 32: the two pieces are the one store's left half and rl_copy_rows of its right half; Y also
    accumulates, out2 never does; memory behind the last row stays untouched."""
    from randlanet import _hip as H
    ops = settings
    K, N, h = 8, 64, 32
    g = torch.Generator().manual_seed(M)
    G = torch.randn((M, K), generator=g).to(DEV)
    W = (torch.randn((K, N), generator=g) * 0.3).to(DEV)         # (K, N): w_ks = N, w_ns = 1
    a = ops.plain(G, 1, M)
    assert ops.gemm_split_supported(a, W, N, 1, N, h, None)
    full = ops.gemm(a, W, N, 1, N, None)
    assert H.lib().rl_last_kernel() == b"sgemm_kernel"
    right = torch.empty((M, N - h), device=DEV)
    ops.copy_rows(full, (h, N - h), M, right, (0, N - h), M, M)
    left = full[:, :h].contiguous()
    Yp, R2 = torch.full((M + 8, h), -7.0, device=DEV), torch.full((M + 8, N - h), -9.0, device=DEV)
    ops.gemm(a, W, N, 1, N, None, out=Yp, out_bstride=M, out2=R2, split_col=h)
    assert H.lib().rl_last_kernel() == b"sgemm_kernel<split>"
    torch.cuda.synchronize()
    assert float(left.abs().max()) > 0 and float(right.abs().max()) > 0
    assert torch.equal(Yp[:M].view(torch.int32), left.view(torch.int32)) and bool((Yp[M:] == -7.0).all())
    assert torch.equal(R2[:M].view(torch.int32), right.view(torch.int32)) and bool((R2[M:] == -9.0).all())
    base = torch.randn((M + 8, h), generator=g).to(DEV)
    Ya, R3 = base.clone(), torch.full((M + 8, N - h), -9.0, device=DEV)
    ops.gemm(a, W, N, 1, N, None, out=Ya, out_bstride=M, out2=R3, split_col=h, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(Ya[:M], left + base[:M]) and torch.equal(Ya[M:], base[M:])
    assert torch.equal(R3[:M].view(torch.int32), right.view(torch.int32)) and bool((R3[M:] == -9.0).all())
    # a split the streaming kernel does not store is refused, and nothing is launched
    launches = H.lib().rl_launch_count()
    assert not ops.gemm_split_supported(a, W, N, 1, N, 24, None)
    with pytest.raises(H.HipKernelError, match="split-scatter"):
        ops.gemm(a, W, N, 1, N, None, out=torch.empty((M, 24), device=DEV), out_bstride=M,
                 out2=torch.empty((M, 40), device=DEV), split_col=24)
    assert H.lib().rl_launch_count() == launches


# ---- engine level: layers [16, 64, 128, 256], K = 16, N = 4096, B = 2, the bound at 0 -----------------------------------------
LAYERS, B_, N_, CN = [16, 64, 128, 256], 2, 4096, 3


def _data():
    rs = np.random.RandomState(0)
    x = rs.uniform(0, 1, (B_, N_, 3)).astype(np.float32)
    y = np.floor(x[..., 2] * CN).clip(0, CN - 1).astype(np.int64)
    return x, y, [rs.permutation(N_) for _ in range(3)]


def _step(setting, use_graph):
    from randlanet import _ops as ops
    from randlanet._train import TrainStep
    from randlanet.utils.modules import RandLANet, RandLANetSettings
    x, y, perms = _data()
    ops.set_decoder_cat(setting)
    torch.manual_seed(0)
    net = RandLANet(RandLANetSettings(n_classes=CN, n_points=N_, n_neighbors=16, layer_sizes=LAYERS), DEV)
    net.fc_end[2].p = 0.0
    net.train()
    step = TrainStep(net, B_, N_, loss="dice", lr=1e-2, use_graph=use_graph)
    step.set_batch(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
    step.capture()
    return step, net, perms


@pytest.fixture()
def engine(monkeypatch):
    """The decoder's row bound at 0; counts the entry points a step goes through (the tracer of tests/golden/make_step_trace.py)."""
    from randlanet import _engine
    from randlanet import _hip as H
    from randlanet import _ops as ops
    monkeypatch.setattr(_engine, "DECODER_CAT_IN_PLACE_MIN_ROWS", 0)
    calls = []
    orig = H.check

    def check(rc, what=""):
        calls.append(what)
        return orig(rc, what)
    monkeypatch.setattr(H, "check", check)
    mode0 = ops.get_decoder_cat()
    yield calls
    ops.set_decoder_cat(mode0)


def _same_bytes(a, b, what):
    for key in a:
        x, y = a[key], b[key]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, key)
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), (what, key)


def test_train_steps_and_eval_forward_are_the_same_either_way(engine):
    calls = engine
    got, took = {}, {}
    for setting in ("stored", "in_place"):
        step, net, perms = _step(setting, False)
        calls.clear()
        step.step(perms[0])
        took[setting] = {name: calls.count(name) for name in ("rl_copy_rows_pair", "rl_copy_rows", "rl_gemm", "rl_wgrad_batch")}
        step.step(perms[1])
        torch.cuda.synchronize()
        out = dict(record=step.out.clone(), gradient=step.flat.grad.clone(), parameters=step.flat.param.detach().clone())
        with torch.no_grad():
            logits, ctx = step.engine.forward(step.inp, torch.from_numpy(perms[2]).to(DEV), False, 0.0)
        out["logits"] = logits.clone()
        ctx.tape.clear()
        ctx.keep.clear()
        torch.cuda.synchronize()
        got[setting] = out
    s, p = took["stored"], took["in_place"]
    # four decoder steps: four concats built on the stored path, none in place (what is left builds other operands: the padded
    # input, the small un-fused pooling blocks); the narrow last step's strided gradient copy is gone too
    assert s["rl_copy_rows_pair"] - p["rl_copy_rows_pair"] == 4, took
    assert s["rl_copy_rows"] - p["rl_copy_rows"] == 1, took
    assert s["rl_gemm"] == p["rl_gemm"], took
    assert torch.isfinite(got["stored"]["gradient"]).all() and float(got["stored"]["gradient"].abs().max()) > 0
    _same_bytes(got["in_place"], got["stored"], "eager")


def test_no_decoder_concat_is_built_in_place(engine, monkeypatch):
    """The decoder's rl_copy_rows_pair calls (the gathered source comes first in them) as the engine issues them."""
    from randlanet import _ops as ops
    seen = []
    pair = ops.copy_rows_pair

    def c_pair(a, b):
        if a[1].get("index") is not None and b[1].get("index") is None:      # (the padded input's pair gathers both)
            seen.append(a[0][1][1] + b[0][1][1])
        return pair(a, b)
    monkeypatch.setattr(ops, "copy_rows_pair", c_pair)
    for setting, want in (("stored", [1024, 512, 256, 64]), ("in_place", [])):
        step, net, perms = _step(setting, False)
        seen.clear()
        step.step(perms[0])
        torch.cuda.synchronize()
        assert seen == want, (setting, seen)


def test_replayed_graph_is_the_same(engine):
    got = {}
    for setting in ("stored", "in_place"):
        step, net, perms = _step(setting, True)
        for p in perms[:2]:
            step.step(p)
        torch.cuda.synchronize()
        got[setting] = dict(record=step.out.clone(), gradient=step.flat.grad.clone(), parameters=step.flat.param.detach().clone())
    assert torch.isfinite(got["stored"]["gradient"]).all()
    _same_bytes(got["in_place"], got["stored"], "graph")


def test_default_bound_keeps_small_concats_stored():
    from randlanet import _engine
    assert 8192 <= _engine.DECODER_CAT_IN_PLACE_MIN_ROWS < 20480, "8192-row concats stay stored; the flagship's 20480 rows lie above"
