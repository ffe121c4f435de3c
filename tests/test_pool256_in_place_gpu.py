"""The d = 256 pooling block (the un-fused path) without a stored X, at step level.

TrainStep with a 256-wide level under rl_set_pool256_x("in_place") and ("stored"): two steps (the second one's forward sees the
first one's gradients) give the same loss record, flat gradient, parameters and BatchNorm running statistics byte for byte, and
the same eval logits.  Once more with a 512-wide level behind it (six concat-gather weight gradients: two grouped launches).
Under the fp32 arithmetic mode and under bf16 storage the engine takes the stored path without an error.

The engine reads X in place only above _engine.POOL_X_IN_PLACE_MIN_ROWS = 2048 rows (the one measured size at which the in-place
form loses, and the size of the blocks whose stored-path launch schedule tests/test_schedule_gpu.py pins - see the constant).
The two configurations the path was specified with have 1024-row and 256-row blocks, below that bound, so their fixture sets
the bound to 0; test_default_bound_takes_a_block_above_it_in_place runs a 3072-row block with nothing patched, and
test_small_blocks_keep_the_stored_path checks the bound itself.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _run(layers, B, N, setting, counts):
    """Two training steps and an eval forward; returns the tensors to compare as int32 views (bytes, not values)."""
    from randlanet import _ops as ops
    from randlanet._train import TrainStep
    from randlanet.utils.modules import RandLANet, RandLANetSettings
    Cn, K = 3, 16
    rs = np.random.RandomState(0)
    x = rs.uniform(0, 1, (B, N, 3)).astype(np.float32)
    y = np.floor(x[..., 2] * Cn).clip(0, Cn - 1).astype(np.int64)
    perms = [rs.permutation(N) for _ in range(3)]
    ops.set_pool256_x(setting)
    torch.manual_seed(0)
    net = RandLANet(RandLANetSettings(n_classes=Cn, n_points=N, n_neighbors=K, layer_sizes=layers), DEV)
    net.fc_end[2].p = 0.0
    net.train()
    step = TrainStep(net, B, N, loss="dice", lr=1e-2, use_graph=False)
    step.set_batch(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
    step.capture()
    counts.clear()
    for p in perms[:2]:
        step.step(p)
    torch.cuda.synchronize()
    rec, grad, param = step.out.clone(), step.flat.grad.clone(), step.flat.param.detach().clone()
    running = torch.cat([v.detach().reshape(-1).float() for k, v in sorted(net.state_dict().items()) if "running" in k])
    taken = dict(counts)
    perm = torch.from_numpy(perms[2]).to(DEV)
    with torch.no_grad():
        logits, ctx = step.engine.forward(step.inp, perm, False, 0.0)
    logits = logits.clone()
    ctx.tape.clear()
    ctx.keep.clear()
    torch.cuda.synchronize()
    return dict(record=rec, gradient=grad, parameters=param, running=running, logits=logits), taken


def _counted(monkeypatch, bound):
    """Counts what the un-fused pooling path launches: stored copies, in-place products / poolings / weight gradients.
    bound: the engine's row bound for the test (None: as it stands)."""
    from randlanet import _ops as ops
    counts = {}
    pair, gemm, fwd, bwd, wgrad = ops.copy_rows_pair, ops.gemm, ops.attpool_fwd, ops.attpool_bwd, ops.wgrad

    def bump(key):
        counts[key] = counts.get(key, 0) + 1

    def c_pair(a, b):
        if b[1].get("index") is not None and b[0][1][1] >= 128:
            bump("copy")
        return pair(a, b)

    def c_gemm(a, *args, **kw):
        if isinstance(a, ops.ConcatGather):
            bump("gemm")
        return gemm(a, *args, **kw)

    def c_fwd(X, *args, **kw):
        bump("fwd_cat" if isinstance(X, ops.ConcatGather) else "fwd")
        return fwd(X, *args, **kw)

    def c_bwd(X, *args, **kw):
        bump("bwd_cat" if isinstance(X, ops.ConcatGather) else "bwd")
        return bwd(X, *args, **kw)

    def c_wgrad(a, dY, dyb, N, *args, **kw):
        if isinstance(a, ops.ConcatGather) and N >= 256:
            bump("wgrad_cat")
        return wgrad(a, dY, dyb, N, *args, **kw)

    for name, fn in (("copy_rows_pair", c_pair), ("gemm", c_gemm), ("attpool_fwd", c_fwd), ("attpool_bwd", c_bwd), ("wgrad", c_wgrad)):
        monkeypatch.setattr(ops, name, fn)
    if bound is not None:
        from randlanet import _engine
        monkeypatch.setattr(_engine, "POOL_X_IN_PLACE_MIN_ROWS", bound)
    mode0, wide0, st0 = ops.get_pool256_x(), ops.get_wide_gemm(), ops.get_storage()
    yield counts
    ops.set_storage("f32")
    ops.set_wide_gemm(wide0)
    ops.set_storage(st0)
    ops.set_pool256_x(mode0)


@pytest.fixture()
def counted(monkeypatch):
    yield from _counted(monkeypatch, 0)


@pytest.fixture()
def counted_default(monkeypatch):
    yield from _counted(monkeypatch, None)


def _same_bytes(a, b, what):
    for key in a:
        x, y = a[key], b[key]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, key)
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), (what, key)


@pytest.mark.parametrize("layers,B,N,blocks", [([16, 64, 128, 256], 2, 2048, 2), ([16, 64, 128, 256, 512], 1, 4096, 4)])
def test_train_step_is_the_same_either_way(counted, layers, B, N, blocks):
    stored, took_s = _run(layers, B, N, "stored", counted)
    assert took_s.get("copy", 0) == 2 * blocks and "gemm" not in took_s and "fwd_cat" not in took_s and "wgrad_cat" not in took_s
    placed, took_p = _run(layers, B, N, "in_place", counted)
    # two steps: every un-fused block's product, pooling, pooling backward and weight gradient read X in place, none stores it
    assert took_p == {"gemm": 2 * blocks, "fwd_cat": 2 * blocks, "bwd_cat": 2 * blocks, "wgrad_cat": 2 * blocks}, took_p
    assert torch.isfinite(stored["gradient"]).all() and float(stored["gradient"].abs().max()) > 0
    _same_bytes(placed, stored, layers)


def test_default_bound_takes_a_block_above_it_in_place(counted_default):
    """layers [16, 64, 128, 256], N = 4096, B = 3: the d = 256 blocks have 3 * 64 * 16 = 3072 rows, above the bound as it stands -
    nothing is patched, the in-place path is the engine's own choice, and the step is the stored one's byte for byte."""
    from randlanet import _engine
    layers, B, N = [16, 64, 128, 256], 3, 4096
    assert B * (N // 64) * 16 > _engine.POOL_X_IN_PLACE_MIN_ROWS
    stored, took_s = _run(layers, B, N, "stored", counted_default)
    assert took_s.get("copy", 0) == 4 and not any(k in took_s for k in ("gemm", "fwd_cat", "bwd_cat", "wgrad_cat")), took_s
    placed, took_p = _run(layers, B, N, "in_place", counted_default)
    assert took_p == {"gemm": 4, "fwd_cat": 4, "bwd_cat": 4, "wgrad_cat": 4}, took_p
    _same_bytes(placed, stored, "default bound")


def test_small_blocks_keep_the_stored_path(monkeypatch):
    """layers [16, 64, 128, 256], N = 2048, B = 2: the d = 256 blocks have 2 * 32 * 16 = 1024 rows.  With the bound at 1024 rows
    they are stored, with 1023 they are read in place; the default bound lies above both."""
    from randlanet import _engine
    assert 1024 < _engine.POOL_X_IN_PLACE_MIN_ROWS < 81920, "the flagship block (81920 rows) must lie above the bound"
    from randlanet import _ops as ops
    counts = {}
    copy, gemm = ops.copy_rows_pair, ops.gemm

    def c_pair(a, b):
        if b[1].get("index") is not None and b[0][1][1] >= 128:
            counts["copy"] = counts.get("copy", 0) + 1
        return copy(a, b)

    def c_gemm(a, *args, **kw):
        if isinstance(a, ops.ConcatGather):
            counts["gemm"] = counts.get("gemm", 0) + 1
        return gemm(a, *args, **kw)

    mode0 = ops.get_pool256_x()
    try:
        monkeypatch.setattr(ops, "copy_rows_pair", c_pair)
        monkeypatch.setattr(ops, "gemm", c_gemm)
        outs = {}
        for bound in (None, 1024, 1023):
            if bound is not None:
                monkeypatch.setattr(_engine, "POOL_X_IN_PLACE_MIN_ROWS", bound)
            outs[bound], took = _run([16, 64, 128, 256], 2, 2048, "in_place", counts)      # (took: the two training steps)
            if bound == 1023:
                assert took == {"gemm": 4}, (bound, took)
            else:
                assert took == {"copy": 4}, (bound, took)
        _same_bytes(outs[1023], outs[1024], "bound")
        _same_bytes(outs[None], outs[1024], "default bound")
    finally:
        ops.set_pool256_x(mode0)


def test_replayed_graph_is_the_same(counted):
    """The captured step replays the in-place launches (the default path of the benchmark)."""
    from randlanet import _ops as ops
    from randlanet._train import TrainStep
    from randlanet.utils.modules import RandLANet, RandLANetSettings
    layers, B, N, Cn = [16, 64, 128, 256], 2, 2048, 3
    rs = np.random.RandomState(0)
    x = rs.uniform(0, 1, (B, N, 3)).astype(np.float32)
    y = np.floor(x[..., 2] * Cn).clip(0, Cn - 1).astype(np.int64)
    perms = [rs.permutation(N) for _ in range(2)]
    got = {}
    for setting in ("stored", "in_place"):
        ops.set_pool256_x(setting)
        torch.manual_seed(0)
        net = RandLANet(RandLANetSettings(n_classes=Cn, n_points=N, n_neighbors=16, layer_sizes=layers), DEV)
        net.fc_end[2].p = 0.0
        net.train()
        step = TrainStep(net, B, N, loss="dice", lr=1e-2, use_graph=True)
        step.set_batch(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
        step.capture()
        for p in perms:
            step.step(p)
        torch.cuda.synchronize()
        got[setting] = dict(record=step.out.clone(), gradient=step.flat.grad.clone(), parameters=step.flat.param.detach().clone())
    _same_bytes(got["in_place"], got["stored"], "graph")


@pytest.mark.parametrize("change", ["fp32 arithmetic", "bf16 storage"])
def test_other_modes_keep_the_stored_path(counted, change):
    from randlanet import _ops as ops
    if change == "fp32 arithmetic":
        ops.set_wide_gemm("fp32")
    else:
        ops.set_storage("bf16")
    out, took = _run([16, 64, 128, 256], 2, 2048, "in_place", counted)
    assert took.get("copy", 0) == 4 and not any(k in took for k in ("gemm", "fwd_cat", "bwd_cat", "wgrad_cat")), took
    assert torch.isfinite(out["gradient"]).all() and torch.isfinite(out["logits"]).all()
