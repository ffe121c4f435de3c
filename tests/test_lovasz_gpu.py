"""The Lovasz-Softmax kernels (csrc/lovasz.hip behind ops.loss_forward / loss_backward, kinds 3 and 4) against their
specification, the numpy twin randlanet/utils/lovasz.py (held to Berman's formula in test_lovasz_cpu.py), and the layers above.

Bounds.  coef: bit for bit - every coefficient is one float64 expression of exact integers, rounded once.  Loss within
1e-12 * max(1, |loss|): float64 sums of at most 2^13 non-negative terms per chunk, regrouped.  dlogits within the project's
1e-4 * max|ref| + 1e-9 (test_masked_loss_gpu.py); exact zeros at unlabelled points; coef exactly 0 at unlabelled points
and absent classes.  out[1:] is the masked cross entropy's record bit for bit.  Inputs: lovasz_inputs.py, wide_inputs.py."""
import numpy as np
import pytest
import torch

import lovasz_inputs as LI
import wide_inputs as WI

pytestmark = pytest.mark.gpu
DEV = "cuda"
_wide = {}


@pytest.fixture(scope="module")
def ops():
    from randlanet import _ops
    return _ops


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _wide_case(mode):
    """wide_inputs.inputs(40) = (3, 40, 700) in one of its three modes, and the twin's result - computed once."""
    from randlanet.utils.lovasz import lovasz_softmax_host
    if mode not in _wide:
        z, y, w = WI.mode_inputs(40, mode)
        _wide[mode] = ((z, y, w), lovasz_softmax_host(z, y, w))
    return _wide[mode]


def _case(name):
    if name.startswith("wide40-"):
        return _wide_case(name[7:])
    return LI.case(name), LI.twin(name)


def _run(ops, z, y, w, name="lovasz"):
    kind = ops.LOSS_KINDS[name][0]
    zd, yd, wd = _dev(z), _dev(y), _dev(w)
    out, work, cf = ops.loss_forward(zd, yd, kind, 0.0, 0.0, True, class_weights=wd, return_coef=True)
    g = ops.loss_backward(zd, yd, kind, 0.0, 0.0, True, work, class_weights=wd)
    return out, g, cf


KERNEL_CASES = LI.GPU_CASES + tuple(f"wide40-{m}" for m in WI.MODES)


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_kernels_against_the_twin(ops, name):
    (z, y, w), (ref_loss, ref_grad, ref_coef) = _case(name)
    B, C, N = z.shape
    out, g, cf = _run(ops, z, y, w)
    loss, gh, ch = float(out[0]), g.cpu().numpy(), cf.cpu().numpy()
    err_l, err_g = abs(loss - ref_loss), float(np.abs(gh - ref_grad).max())
    print(f"[lovasz] {name} {z.shape}: loss {loss:.15f} / {ref_loss:.15f} (diff {err_l:.2e}), gradient diff {err_g:.2e} of max "
          f"{np.abs(ref_grad).max():.2e}, {int(np.count_nonzero(ch.view(np.uint32) != ref_coef.view(np.uint32)))} coefficients differ")
    assert ch.shape == ref_coef.shape == (C, B * N)
    assert np.array_equal(ch.view(np.uint32), ref_coef.view(np.uint32))         # bit for bit
    assert err_l <= 1e-12 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    assert err_g <= 1e-4 * np.abs(ref_grad).max() + 1e-9, err_g
    ok = (y >= 0) & (y < C)
    dead = g.permute(0, 2, 1)[~_dev(ok)]
    assert torch.equal(dead, torch.zeros_like(dead))                            # unlabelled points: exact zeros, written
    assert not ch[:, ~ok.reshape(-1)].any()
    assert not ch[np.bincount(y[ok], minlength=C) == 0].any()                   # absent classes
    if name in ("unlabelled", "zero_weight_sum"):
        assert loss == 0.0 and not gh.any()
    # the record's counts: the masked cross entropy's, bit for bit
    ce, _ = ops.loss_forward(_dev(z), _dev(y), 0, 0.0, 0.0, True, class_weights=_dev(w), ignore_unlabelled=True)
    assert torch.equal(out[1:], ce[1:])


@pytest.mark.parametrize("name", ["rand13", "mixed7", "sat40", "unlabelled", "wide40-weighted"])
def test_the_sum_with_cross_entropy(ops, name):
    from randlanet.utils.lovasz import masked_cross_entropy_host
    (z, y, w), (ref_loss, ref_grad, ref_coef) = _case(name)
    out, g, cf = _run(ops, z, y, w, "lovasz_cross_entropy")
    lov, _, _ = _run(ops, z, y, w, "lovasz")
    zd, yd, wd = _dev(z), _dev(y), _dev(w)
    ce, ce_work = ops.loss_forward(zd, yd, 0, 0.0, 0.0, True, class_weights=wd, ignore_unlabelled=True)
    assert float(out[0]) == float(lov[0]) + float(ce[0])                        # the fp64 sum of the two losses
    assert torch.equal(out[1:], ce[1:])
    assert np.array_equal(cf.cpu().numpy().view(np.uint32), ref_coef.view(np.uint32))
    _, ce_grad = masked_cross_entropy_host(z, y, None if w is None else w.astype(np.float64))
    ref = ref_grad + ce_grad
    err = float(np.abs(g.cpu().numpy() - ref).max())
    print(f"[lovasz + ce] {name}: loss {float(out[0]):.12f}, gradient diff {err:.2e} of max {np.abs(ref).max():.2e}")
    assert err <= 1e-4 * np.abs(ref).max() + 1e-9, err
    ok = (y >= 0) & (y < z.shape[1])
    dead = g.permute(0, 2, 1)[~_dev(ok)]
    assert torch.equal(dead, torch.zeros_like(dead))


@pytest.mark.parametrize("name", ["rand13", "ties13", "wide40-weighted"])
def test_two_runs_are_bitwise_equal(ops, name):
    (z, y, w), _ = _case(name)
    for loss in ("lovasz", "lovasz_cross_entropy"):
        a = _run(ops, z, y, w, loss)
        a = [t.clone() for t in a]
        b = _run(ops, z, y, w, loss)
        assert all(torch.equal(s.view(torch.int32) if s.dtype == torch.float32 else s.view(torch.int64),
                               t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64)) for s, t in zip(a, b))


def test_a_workspace_is_reused_and_the_module_runs(ops):
    """`work=`: the same workspace for inputs with different numbers of labelled points, stale contents and all; and the
    autograd module on top."""
    from randlanet.utils.losses import get_loss
    (z, y, w), (ref_loss, ref_grad, ref_coef) = _case("mixed7")
    B, C, N = z.shape
    zd, wd = _dev(z), _dev(w)
    ws = ops.lovasz_workspace(DEV, B, C, N)
    ws.fill_(0xA5)
    y2 = y.copy()
    y2[0, ::3] = -1
    out2, _ = ops.loss_forward(zd, _dev(y2), 3, 0.0, 0.0, True, class_weights=wd, work=ws)
    out2 = out2.clone()
    out, work, cf = ops.loss_forward(zd, _dev(y), 3, 0.0, 0.0, True, class_weights=wd, work=ws, return_coef=True)
    assert work is ws and float(out2[0]) != float(out[0])
    assert abs(float(out[0]) - ref_loss) <= 1e-12 and np.array_equal(cf.cpu().numpy().view(np.uint32), ref_coef.view(np.uint32))
    for name, ref in (("lovasz", ref_loss),):
        crit = get_loss(name, class_weights=w).to(DEV)
        lt = _dev(z).requires_grad_(True)
        loss = crit(lt, _dev(y))
        (3.0 * loss).backward()
        assert abs(float(loss.detach()) - np.float32(ref)) <= 1e-7
        assert float((lt.grad.cpu().double() - 3.0 * torch.from_numpy(ref_grad)).abs().max()) <= 3e-4 * np.abs(ref_grad).max() + 3e-9


def test_refusals_launch_nothing(ops):
    """C = 257, B*N*C >= 2^31, a small workspace and sync= are refused and nothing is launched (modelled on
    test_wide_classes_gpu.test_257_classes_are_refused_and_nothing_is_launched); the rl_loss_* / rl_head_* entries keep
    refusing the kinds they do not know."""
    H = ops.H
    lib = H.lib()
    C, n = 257, 64
    logits = torch.zeros((1, C, n), device=DEV)
    labels = torch.zeros((1, n), dtype=torch.int64, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    out = torch.full((1 + 4 * C,), -1.0, dtype=torch.float64, device=DEV)
    g = torch.full((1, C, n), -1.0, device=DEV)
    lp, yp, wp, op, gp, st = logits.data_ptr(), labels.data_ptr(), ws.data_ptr(), out.data_ptr(), g.data_ptr(), ops._st()
    n0 = lib.rl_launch_count()
    codes = [lib.rl_lovasz_forward(lp, yp, 1, C, n, 0, None, wp, ws.numel(), op, st),
             lib.rl_lovasz_forward(lp, yp, 1, C, n, 1, None, wp, ws.numel(), op, st),
             lib.rl_lovasz_backward(lp, yp, 1, C, n, 0, None, wp, ws.numel(), 1.0, gp, st),
             lib.rl_lovasz_backward(lp, yp, 1, C, n, 1, None, wp, ws.numel(), 1.0, gp, st)]
    assert codes == [-4] * 4, codes                     # RL_ERR_UNSUPPORTED
    assert "257" in lib.rl_last_error().decode() and "256" in lib.rl_last_error().decode()
    assert lib.rl_lovasz_forward(lp, yp, 2 ** 15, 2, 2 ** 15, 0, None, wp, ws.numel(), op, st) == -4       # 2^31 keys (sizes only)
    assert lib.rl_lovasz_forward(lp, yp, 1, 2, n, 0, None, wp, 1024, op, st) == -1                         # small workspace
    assert lib.rl_lovasz_backward(lp, yp, 1, 2, n, 0, None, wp, 1024, 1.0, gp, st) == -1
    assert lib.rl_lovasz_forward(lp, yp, 1, 2, n, 0, None, wp, ws.numel(), None, st) == -1                 # null out
    # the unsorted entries do not know the new kinds
    work = torch.zeros(lib.rl_loss_work_doubles(n, 2), dtype=torch.float64, device=DEV)
    for kind in (3, 4):
        assert lib.rl_loss_forward(lp, yp, 1, 2, n, kind, 0.5, 1.0, 1, work.data_ptr(), op, st) == -1
        assert lib.rl_loss_forward_masked(lp, yp, 1, 2, n, kind, 0.5, 1.0, 1, None, 1, work.data_ptr(), op, st) == -1
        assert lib.rl_loss_backward(lp, yp, 1, 2, n, kind, 0.5, 1.0, 1, work.data_ptr(), 1.0, gp, st) == -1
        assert lib.rl_loss_backward_masked(lp, yp, 1, 2, n, kind, 0.5, 1.0, 1, work.data_ptr(), 1.0, None, 1, gp, st) == -1
    assert lib.rl_launch_count() == n0
    torch.cuda.synchronize()
    assert bool((out == -1.0).all()) and bool((g == -1.0).all()) and not ws.any() and not work.any()

    class FakeSync:
        world = 1

    small = torch.zeros((1, 2, n), device=DEV)
    for kind in (3, 4):
        with pytest.raises(H.HipKernelError, match="sync="):
            ops.loss_forward(small, labels, kind, 0.0, 0.0, True, sync=FakeSync())
        with pytest.raises(H.HipKernelError, match="sync="):
            ops.loss_backward(small, labels, kind, 0.0, 0.0, True, ws, sync=FakeSync())
        with pytest.raises(H.HipKernelError):
            ops.loss_forward(logits, labels, kind, 0.0, 0.0, True)          # 257 classes
    with pytest.raises(H.HipKernelError):
        ops.loss_forward(small, labels, 5, 0.0, 0.0, True)                  # no such kind
    assert lib.rl_launch_count() == n0


# ----------------------------------------------------------------------------------------------------------- network cases
K, LAYERS = 16, [8, 16, 32, 32]


def _net(C, N, seed=0):
    from randlanet.utils.modules import RandLANet, RandLANetSettings
    torch.manual_seed(seed)
    net = RandLANet(RandLANetSettings(n_classes=C, n_points=N, n_neighbors=K, layer_sizes=LAYERS), DEV)
    net.fc_end[2].p = 0.0
    net.train()
    return net


def test_train_step_is_the_manual_composition(ops, monkeypatch):
    """TrainStep(loss="lovasz") at C = 5 - where the fused head exists - in the eager schedule: its record and every parameter
    gradient equal, bit for bit, engine.forward(head=None) -> loss_forward(kind 3) -> loss_backward -> engine.backward on a
    second network built from the same seed.  The fused head stepped aside (it is never called), and the step's static
    workspace gives what a fresh one gives."""
    from randlanet._train import TrainStep
    C, Bn, Nn = 5, 2, 2051
    rs = np.random.RandomState(2)
    x = rs.uniform(0, 1, (Bn, Nn, 3)).astype(np.float32)
    y = np.floor(x[..., 2] * C).clip(0, C - 1).astype(np.int64)
    perm = rs.permutation(Nn)
    assert ops.H.lib().rl_head_supported(C, 32)
    fused = []
    head_fwd = ops.head_fwd
    monkeypatch.setattr(ops, "head_fwd", lambda *a, **k: (fused.append(1), head_fwd(*a, **k))[1])
    res = {}
    for how in ("step", "manual"):
        st = TrainStep(_net(C, Nn), Bn, Nn, loss="lovasz", use_graph=False)
        assert st.kind == 3 and st._loss_ws is not None
        st.set_batch(_dev(x), _dev(y))
        st.perm.copy_(_dev(perm))
        if how == "step":
            st._fwd_bwd()
            rec = st.out
        else:
            logits, ctx = st.engine.forward(st.inp, st.perm, True, 0.0, head=None)
            assert tuple(logits.shape) == (Bn, C, Nn)
            rec, work = ops.loss_forward(logits, st.labels, 3, 0.0, 0.0, True)
            dlogits = ops.loss_backward(logits, st.labels, 3, 0.0, 0.0, True, work)
            st.engine.backward(ctx, dlogits, st.flat.grads)
        torch.cuda.synchronize()
        res[how] = (rec.clone(), {n: g.detach().clone() for n, g in st.flat.grads.items()})
    assert not fused
    (rec, grads), (rec_m, grads_m) = res["step"], res["manual"]
    assert bool(torch.isfinite(rec).all()) and 0.0 < float(rec[0]) <= 1.0
    assert torch.equal(rec, rec_m)
    for n, g in grads.items():
        assert torch.equal(g, grads_m[n]), n
    assert any(bool(g.any()) for g in grads.values())


@pytest.mark.parametrize("C", [5, 40])
def test_train_step_graph_replay_equals_eager_schedule(C):
    """test_train_step_graph_replay_equals_eager_schedule_at_40_classes' statement with the sorted loss in the captured step,
    the batch swapped at step 3 for one with another number of labelled points: P is device state, the graph follows it."""
    from randlanet._train import TrainStep
    Bn, Nn = 2, 2048
    rs = np.random.RandomState(0)
    x = rs.uniform(0, 1, (Bn, Nn, 3)).astype(np.float32)
    y = np.floor(x[..., 2] * C).clip(0, C - 1).astype(np.int64)
    y[rs.uniform(size=y.shape) < 0.3] = -1
    x2 = x[::-1].copy()
    y2 = np.floor(x2[..., 2] * C).clip(0, C - 1).astype(np.int64)
    y2[rs.uniform(size=y.shape) < 0.6] = C + 1
    assert np.count_nonzero(y >= 0) != np.count_nonzero(y2 < C)
    perms = [rs.permutation(Nn) for _ in range(6)]
    records, weights = {}, {}
    for mode in ("graph", "eager"):
        net = _net(C, Nn)
        step = TrainStep(net, Bn, Nn, loss="lovasz", lr=1e-2, use_graph=mode == "graph", ignore_unlabelled=True)
        step.set_batch(_dev(x), _dev(y))
        step.capture()
        rec = []
        for i, p in enumerate(perms):
            if i == 3:
                step.set_batch(_dev(x2), _dev(y2))
            step.step(p)
            rec.append(step.out.clone())
        torch.cuda.synchronize()
        records[mode] = torch.stack(rec).cpu()
        weights[mode] = step.flat.param.detach().cpu().clone()
    assert bool(torch.isfinite(records["graph"]).all())
    labelled = records["graph"][:, 1 + C:1 + 2 * C].sum(1)
    assert labelled[0] == np.count_nonzero(y >= 0) and labelled[3] == np.count_nonzero(y2 < C)
    assert torch.equal(records["graph"], records["eager"]) and torch.equal(weights["graph"], weights["eager"])


def test_forty_adam_steps_lower_the_loss():
    """40 Adam steps with "lovasz" on labels that are a function of z: the mean loss of the last five records is below that
    of the first five (a deterministic run)."""
    from randlanet._train import TrainStep
    C, Bn, Nn = 5, 2, 1024
    rs = np.random.RandomState(4)
    x = rs.uniform(0, 1, (Bn, Nn, 3)).astype(np.float32)
    y = np.floor(x[..., 2] * C).clip(0, C - 1).astype(np.int64)
    net = _net(C, Nn, seed=1)
    step = TrainStep(net, Bn, Nn, loss="lovasz", lr=1e-2, use_graph=True)
    step.set_batch(_dev(x), _dev(y))
    step.capture()
    rec = []
    for _ in range(40):
        step.step(rs.permutation(Nn))
        rec.append(step.out[:1].clone())
    losses = torch.cat(rec).cpu().numpy()
    print(f"[lovasz training] first five {losses[:5].round(4)}, last five {losses[-5:].round(4)}")
    assert np.all(np.isfinite(losses)) and losses[-5:].mean() < losses[:5].mean()


def _scene40():
    rs = np.random.RandomState(5)
    xyz = rs.uniform((0, 0, -1), (3, 3, 1), (6000, 3)).astype(np.float32)
    labels = np.floor((xyz[:, 2] + 1) / 2 * 40).clip(0, 39).astype(np.int64)
    labels[rs.uniform(size=6000) < 0.3] = -1                    # partly labelled
    return xyz, np.zeros((6000, 0), np.float32), labels


def test_train_scenes_and_evaluate_with_the_sorted_losses():
    from randlanet import AugmentationSettings, Model, RandLANetSettings, TrainingSettings
    torch.manual_seed(0)
    np.random.seed(0)
    names = [f"class {c}" for c in range(40)]
    model = Model(RandLANetSettings(n_classes=40, n_points=2048, n_neighbors=8, layer_sizes=[8, 16, 32, 32]))
    hist = []
    scene = _scene40()
    model.train_scenes([scene], [scene], TrainingSettings(epochs=2, batch_size=2, learning_rate=1e-2, early_stopping=False,
                                                          ignore_unlabelled=True, loss_function="lovasz_cross_entropy"),
                       AugmentationSettings(), crops_per_epoch=4, validation_crops=2, seed=3, class_names=names,
                       callbacks=[lambda e, m: hist.append((m["loss"], m["val_loss"]))], pad_small_scenes=False)
    assert len(hist) == 2 and np.all(np.isfinite(hist)), hist
    rs = np.random.RandomState(9)
    data = []
    for _ in range(2):
        xyz = rs.uniform(0, 1, (2500, 3)).astype(np.float32)
        data.append((xyz, np.zeros((2500, 0), np.float32), np.floor(xyz[:, 2] * 40).clip(0, 39).astype(np.int64)))
    res = model.evaluate(data, names, batch_size=2, loss_function="lovasz")
    assert np.isfinite(res["loss"]) and 0.0 <= res["loss"] <= 1.0, res["loss"]
