"""The masked loss mode in the fused head (rl_head_fwd / rl_head_bwd) and in the captured training step: the fused path against
the separate launches with test_fused_head_equals_the_separate_launches' network, bounds and exclusions, and graph replay
against the eager schedule over batches with different numbers of unlabelled points."""
import numpy as np
import pytest
import torch

import masked_inputs as MI

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, K, LAYERS, B = 2051, 16, [8, 16, 32, 32], 3


def _weights(labels, C):
    from randlanet.utils.losses import class_weights_from_labels
    return class_weights_from_labels([labels], C)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("loss_name,p_drop,C", [("cross_entropy", 0.0, 3), ("dice", 0.5, 3), ("focal", 0.5, 9),
                                                ("cross_entropy", 0.3, 13), ("focal_tversky", 0.0, 32)])
def test_masked_fused_head_equals_the_separate_launches(loss_name, p_drop, C, weighted, monkeypatch):
    from randlanet import _ops as ops
    from randlanet._train import TrainStep
    from randlanet.utils.modules import RandLANet, RandLANetSettings
    rs = np.random.RandomState(1)
    x = torch.from_numpy(rs.uniform(0, 1, (B, N, 3)).astype(np.float32)).to(DEV)
    labels = MI.recipe_labels(B, N, C)
    MI.check_recipe(labels, C)
    y = torch.from_numpy(labels).to(DEV)
    perm = torch.from_numpy(rs.permutation(N)).to(DEV)
    w = _weights(labels, C) if weighted else None
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, "NO_FUSED_HEAD", not fused)
        torch.manual_seed(5)
        net = RandLANet(RandLANetSettings(n_classes=C, n_points=N, n_neighbors=K, layer_sizes=LAYERS), DEV)
        net.fc_end[2].p = p_drop
        net.train()
        st = TrainStep(net, B, N, loss=loss_name, use_graph=False, class_weights=w, ignore_unlabelled=True)
        st.set_batch(x, y)
        st.perm.copy_(perm)
        n0 = ops.H.lib().rl_launch_count()
        st._fwd_bwd()
        torch.cuda.synchronize()
        res[fused] = (st.out.cpu().numpy().copy(), {n: g.detach().cpu().clone() for n, g in st.flat.grads.items()},
                      ops.H.lib().rl_launch_count() - n0)
    (o1, g1, l1), (o0, g0, l0) = res[True], res[False]
    assert l1 < l0, (l1, l0)                                   # the fused step really took the fused path
    ok = (labels >= 0) & (labels < C)
    np.testing.assert_array_equal(o0[1 + C:1 + 2 * C], np.bincount(labels[ok], minlength=C))      # labelled points only
    assert o1[1 + 2 * C:1 + 3 * C].sum() == ok.sum()                                              # predictions of those only
    np.testing.assert_allclose(o1[0], o0[0], rtol=2e-6, atol=1e-7)             # loss
    np.testing.assert_array_equal(o1[1:1 + 3 * C], o0[1:1 + 3 * C])           # integer counts behind accuracy / IoU
    np.testing.assert_allclose(o1[1 + 3 * C:], o0[1 + 3 * C:], rtol=1e-5)      # sums of probabilities
    worst = (0.0, "")
    for name, a in g0.items():
        if (name.endswith("conv.bias") and not name.startswith("fc_end.3")) or name == "fc_start.bias":
            continue                                           # in front of a BatchNorm: true gradient 0, rounding noise
        assert bool(torch.isfinite(g1[name]).all()), name
        e = float((g1[name] - a).abs().max()) / (float(a.abs().max()) + 1e-12)
        worst = max(worst, (e, name))
    print(f"[masked fused head] {loss_name}, Dropout {p_drop}, C={C}, weighted={weighted}: {l0} -> {l1} launches, "
          f"loss {o1[0]:.7f} / {o0[0]:.7f}, worst relative gradient difference {worst[0]:.1e} ({worst[1]})")
    assert worst[0] < 2e-4, worst


@pytest.mark.parametrize("loss_name,p_drop,C,weighted", [("dice", 0.0, 3, False), ("cross_entropy", 0.3, 13, True)])
def test_masked_graph_replay_follows_the_batch(loss_name, p_drop, C, weighted):
    """The captured step against the eager schedule from the same state over consecutive batches with DIFFERENT numbers of
    unlabelled points - the recipe's half, none labelled at all, every point labelled: record, gradients and updated parameters
    bit for bit.  A normaliser baked into the captured launch arguments would keep the capture batch's value."""
    from randlanet._train import TrainStep
    from randlanet.utils.modules import RandLANet, RandLANetSettings
    rs = np.random.RandomState(2)
    x = torch.from_numpy(rs.uniform(0, 1, (B, N, 3)).astype(np.float32)).to(DEV)
    half = MI.recipe_labels(B, N, C)
    i = np.arange(B * N, dtype=np.int64)
    full = ((7 * i + i // N) % C).reshape(B, N)
    batches = [half, np.full((B, N), -1, np.int64), full, half]
    perms = [rs.permutation(N) for _ in batches]
    w = _weights(half, C) if weighted else None
    runs = {}
    for mode in ("graph", "eager"):
        torch.manual_seed(0)
        net = RandLANet(RandLANetSettings(n_classes=C, n_points=N, n_neighbors=K, layer_sizes=LAYERS), DEV)
        net.fc_end[2].p = p_drop
        net.train()
        step = TrainStep(net, B, N, loss=loss_name, lr=1e-2, use_graph=mode == "graph", class_weights=w, ignore_unlabelled=True)
        step.set_batch(x, torch.from_numpy(full).to(DEV))          # captured on a batch without unlabelled points
        step.capture()
        assert (step._g_main is not None) == (mode == "graph")
        rec = []
        for lab, p in zip(batches, perms):
            step.set_batch(x, torch.from_numpy(lab).to(DEV))
            step.step(p)
            rec.append((step.out.clone(), step.flat.grad.clone(), step.flat.param.detach().clone()))
        torch.cuda.synchronize()
        runs[mode] = rec
    for k, (g, e) in enumerate(zip(runs["graph"], runs["eager"])):
        for what, a, b in zip(("record", "gradients", "parameters"), g, e):
            assert bool(torch.isfinite(a).all()), (k, what)
            assert torch.equal(a, b), (k, what)
    out_none, grad_none = runs["graph"][1][0], runs["graph"][1][1]
    assert float(out_none[0]) == 0.0 and torch.equal(grad_none, torch.zeros_like(grad_none))
    losses = [float(r[0][0]) for r in runs["graph"]]
    assert losses[0] > 0 and losses[2] > 0 and losses[0] != losses[2], losses
    labelled = [float(r[0][1 + C:1 + 2 * C].sum()) for r in runs["graph"]]
    assert labelled == [float(((b >= 0) & (b < C)).sum()) for b in batches], labelled
