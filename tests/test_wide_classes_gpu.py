"""Training and evaluating with 33 .. 256 classes: the wide loss / metric kernels of csrc/loss.hip (lossw_*) behind the unchanged
rl_loss_* entries, and the layers above them.

Yardstick and bounds are those of test_masked_loss_gpu.py: the oracle's loss_by_name on the compacted labelled points in float64
(unweighted), masked_inputs.weighted_twin in float64 (weighted); loss within 2e-6 * max(1, |loss|), gradient within
1e-4 * max|ref| + 1e-9, exact zeros at unlabelled points, integer counts exactly np.bincount / the oracle's accuracy and iou,
sum of probabilities per class within rtol 1e-5.  The yardstick's own fp32 run stays inside a third of each bound on these
inputs (test_wide_classes_cpu.py), so the bounds apply unchanged.  Inputs: wide_inputs.py."""
import numpy as np
import pytest
import torch

import masked_inputs as MI
import wide_inputs as WI

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, N = WI.B, WI.N
_yards = {}


@pytest.fixture(scope="module")
def ops():
    from randlanet import _ops
    return _ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _yard(C, name, mode):
    if (C, name, mode) not in _yards:          # computed once, shared, never modified
        logits, labels, w = WI.mode_inputs(C, mode)
        _yards[(C, name, mode)] = WI.yardstick(name, logits, labels, w)
    return _yards[(C, name, mode)]


def _run(ops, logits, labels, name, weights=None, masked=True, neglect=True):
    kind, alpha, gamma = ops.LOSS_KINDS[name]
    kw = dict(class_weights=weights, ignore_unlabelled=masked)
    out, work = ops.loss_forward(logits, labels, kind, alpha, gamma, neglect, **kw)
    g = ops.loss_backward(logits, labels, kind, alpha, gamma, neglect, work, **kw)
    return out, g, work


def _check_loss_and_gradient(tag, out, g, ref_loss, ref_grad):
    loss = float(out[0])
    gh = g.cpu().numpy()
    err_l, err_g = abs(loss - ref_loss), float(np.abs(gh - ref_grad).max())
    print(f"[wide loss] {tag}: loss {loss:.9f} / {ref_loss:.9f} (diff {err_l:.2e}), "
          f"gradient diff {err_g:.2e} of max {np.abs(ref_grad).max():.2e}")
    assert err_l <= 2e-6 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    assert err_g <= 1e-4 * np.abs(ref_grad).max() + 1e-9, err_g


def _check_counts(out, logits_h, labels_h, C, metrics=True):
    """The record's counts over the labelled points: exactly the integers; sum p within rtol 1e-5; OA / IoU of the oracle."""
    from oracle import loss_metrics_oracle as LM
    ok = (labels_h >= 0) & (labels_h < C)
    cl = np.ascontiguousarray(np.transpose(logits_h, (0, 2, 1))[ok].T)          # (C, n)
    cy = labels_h[ok]
    pred = np.argmax(cl, axis=0)
    cnt = out[1:].cpu().numpy().reshape(4, C)
    np.testing.assert_array_equal(cnt[0], np.bincount(cy[pred == cy], minlength=C).astype(np.float64))
    np.testing.assert_array_equal(cnt[1], np.bincount(cy, minlength=C).astype(np.float64))
    np.testing.assert_array_equal(cnt[2], np.bincount(pred, minlength=C).astype(np.float64))
    p64 = torch.softmax(torch.from_numpy(cl).double(), dim=0).sum(1).numpy()
    np.testing.assert_allclose(cnt[3], p64, rtol=1e-5)
    if metrics:
        oa, pca = LM.accuracy(cl, cy)
        miou, pci = LM.iou(cl, cy)
        assert abs(cnt[0].sum() / cnt[1].sum() - oa) < 1e-7
        for c in range(C):
            union = cnt[1][c] + cnt[2][c] - cnt[0][c]
            assert abs((1.0 if union == 0 else cnt[0][c] / union) - pci[c]) < 1e-7
            assert abs((1.0 if cnt[1][c] == 0 else cnt[0][c] / cnt[1][c]) - pca[c]) < 1e-7


# ------------------------------------------------------------------------------------------------------------ kernel cases
@pytest.mark.parametrize("mode", WI.MODES)
@pytest.mark.parametrize("C", WI.CLASSES)
@pytest.mark.parametrize("name", MI.LOSS_NAMES)
def test_wide_loss_against_the_yardstick(ops, name, C, mode):
    logits_h, labels_h, w32 = WI.mode_inputs(C, mode)
    if mode != "plain":
        WI.check_recipe(labels_h, C)
    logits, labels = _dev(logits_h), _dev(labels_h)
    out, g, _ = _run(ops, logits, labels, name, _dev(w32) if w32 is not None else None, masked=mode != "plain")
    _check_loss_and_gradient(f"{name} C={C} {mode}", out, g, *_yard(C, name, mode))
    _check_counts(out, logits_h, labels_h, C)
    if mode != "plain":         # unlabelled points: exact zeros, written
        ok = (labels_h >= 0) & (labels_h < C)
        dead = g.permute(0, 2, 1)[~_dev(ok)]
        assert dead.numel() > 0 and torch.equal(dead, torch.zeros_like(dead))


@pytest.mark.parametrize("neglect", [True, False], ids=["neglect", "keep"])
@pytest.mark.parametrize("name", sorted(WI.TVERSKY))
def test_empty_classes(ops, name, neglect):
    """C = 64, labels below 32 only: the Tversky terms of classes with tp = sum y = 0, the background neglected and kept."""
    logits_h, labels_h = WI.empty_class_inputs()
    out, g, _ = _run(ops, _dev(logits_h), _dev(labels_h), name, masked=False, neglect=neglect)
    _check_loss_and_gradient(f"{name} C=64, 32 empty classes, neglect={neglect}", out, g,
                             *WI.tversky_twin(logits_h, labels_h, *WI.TVERSKY[name], neglect))
    _check_counts(out, logits_h, labels_h, 64)
    assert not out[1 + 64 + 32:1 + 2 * 64].any()        # no label of an empty class


@pytest.mark.parametrize("name", ["cross_entropy", "dice"])
def test_more_tiles_than_slots(ops, name):
    """B = 1, N = 270000, C = 33: 1055 tiles of 256 rows on RL_MAX_SLOTS = 1024 workgroups - some run two tiles."""
    C, n = 33, 270000
    assert (n + 255) // 256 > ops.H.lib().rl_row_blocks(n, 256) == 1024
    g = torch.Generator().manual_seed(7)
    logits_h = (2.0 * torch.randn((1, C, n), generator=g)).numpy()
    labels_h = WI.base_labels(1, n, C)
    out, grad, _ = _run(ops, _dev(logits_h), _dev(labels_h), name, masked=False)
    _check_loss_and_gradient(f"{name} C={C} N={n}", out, grad, *WI.yardstick(name, logits_h, labels_h))
    _check_counts(out, logits_h, labels_h, C, metrics=False)


class _OneRank:
    """The data-parallel equivalence mode with one rank: the all-reduce of the totals record is the identity."""
    world = 1

    def allreduce(self, t):
        pass

    def global_rows(self, rows):
        return rows


@pytest.mark.parametrize("name", MI.LOSS_NAMES)
def test_partials_and_totals_are_the_forward(ops, name):
    C = 40
    logits_h, labels_h, _ = WI.mode_inputs(C, "plain")
    logits, labels = _dev(logits_h), _dev(labels_h)
    kind, alpha, gamma = ops.LOSS_KINDS[name]
    out, work = ops.loss_forward(logits, labels, kind, alpha, gamma, True)
    g = ops.loss_backward(logits, labels, kind, alpha, gamma, True, work)
    out2, work2 = ops.loss_forward(logits, labels, kind, alpha, gamma, True, sync=_OneRank())
    g2 = ops.loss_backward(logits, labels, kind, alpha, gamma, True, work2, sync=_OneRank())
    o = ops.H.lib().rl_loss_totals_offset(C)
    assert o == 1024 * (5 * C + 1)
    assert torch.equal(work2[o:o + 5 * C + 1], work[o:o + 5 * C + 1])       # the totals record, bitwise
    assert torch.equal(out2, out) and torch.equal(g2, g)


@pytest.mark.parametrize("name", MI.LOSS_NAMES)
def test_two_runs_are_bitwise_equal(ops, name):
    C = 200
    logits_h, labels_h, w32 = WI.mode_inputs(C, "weighted")
    logits, labels, w = _dev(logits_h), _dev(labels_h), _dev(w32)
    a = _run(ops, logits, labels, name, w)
    b = _run(ops, logits, labels, name, w)
    o = ops.H.lib().rl_loss_totals_offset(C)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2][o:], b[2][o:])


def test_257_classes_are_refused_and_nothing_is_launched(ops):
    H = ops.H
    lib = H.lib()
    C, n = 257, 64
    assert lib.rl_loss_max_classes() == 256
    logits = torch.zeros((1, C, n), device=DEV)
    labels = torch.zeros((1, n), dtype=torch.int64, device=DEV)
    work = torch.zeros(lib.rl_loss_work_doubles(n, C), dtype=torch.float64, device=DEV)
    out = torch.full((1 + 4 * C,), -1.0, dtype=torch.float64, device=DEV)
    g = torch.full((1, C, n), -1.0, device=DEV)
    lp, yp, wp, op, gp, st = logits.data_ptr(), labels.data_ptr(), work.data_ptr(), out.data_ptr(), g.data_ptr(), ops._st()
    n0 = lib.rl_launch_count()
    codes = [lib.rl_loss_forward(lp, yp, 1, C, n, 0, 0.5, 1.0, 1, wp, op, st),
             lib.rl_loss_forward_masked(lp, yp, 1, C, n, 0, 0.5, 1.0, 1, None, 1, wp, op, st),
             lib.rl_loss_partials(lp, yp, 1, C, n, 0, 1.0, wp, st),
             lib.rl_loss_from_totals(n, C, 0, 0.5, 1.0, 1, wp, op, st),
             lib.rl_loss_backward(lp, yp, 1, C, n, 0, 0.5, 1.0, 1, wp, 1.0, gp, st),
             lib.rl_loss_backward_masked(lp, yp, 1, C, n, 0, 0.5, 1.0, 1, wp, 1.0, None, 1, gp, st),
             lib.rl_loss_backward_global(lp, yp, 1, C, n, 0, 0.5, 1.0, 1, wp, 1.0, n, gp, st)]
    assert codes == [-4] * 7, codes                     # RL_ERR_UNSUPPORTED
    assert lib.rl_launch_count() == n0
    assert "257" in lib.rl_last_error().decode() and "256" in lib.rl_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == -1.0).all()) and bool((g == -1.0).all()) and not work.any()
    with pytest.raises(H.HipKernelError):
        ops.loss_forward(logits, labels, 0, 0.0, 0.0, True)


# ----------------------------------------------------------------------------------------------------------- network cases
NET = dict(C=40, K=16, layers=[8, 16, 32, 32], B=3)


def test_train_step_at_40_classes_matches_oracle_autograd():
    """_train.TrainStep at n_classes = 40 (the fused head steps aside: Dropout, GEMM, un-permute, wide loss as separate
    launches) against the CPU oracle network under autograd, the way test_configs_gpu.py checks its configurations: loss,
    every parameter gradient within that file's bound for the arithmetic mode, Dropout p = 0.  Metric counts: the label counts
    exactly; predictions can differ from the oracle's only where its two largest logits are closer than twice the 1e-3 the
    logits are held to."""
    from test_configs_gpu import GRAD_BOUND, _check_gradient, _oracle_step, _pair
    from randlanet import _ops as ops
    from randlanet._train import TrainStep
    C, K, layers, Bn = NET["C"], NET["K"], NET["layers"], NET["B"]
    Nn = 2051
    net, sd = _pair(C, Nn, K, layers, seed=41)
    net.fc_end[2].p = 0.0
    net.train()
    rs = np.random.RandomState(3)
    x = rs.uniform(0, 1, (Bn, Nn, 3)).astype(np.float32)
    y = np.floor(rs.uniform(0, 1, (Bn, Nn)) ** 2 * C).clip(0, C - 1).astype(np.int64)
    perm = rs.permutation(Nn)
    ref, ref_loss, g32, _ = _oracle_step(sd, x, y, perm, layers, K)
    st = TrainStep(net, Bn, Nn, loss="dice", use_graph=False)
    assert not ops.H.lib().rl_head_supported(C, 32)
    st.set_batch(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
    st.perm.copy_(torch.from_numpy(perm).to(DEV))
    st._fwd_bwd()
    torch.cuda.synchronize()
    loss = float(st.out[0])
    assert abs(loss - ref_loss) < 1e-5 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    mode = ops.get_wide_gemm()
    worst = 0.0
    for name, _ in net.named_parameters():
        worst = max(worst, _check_gradient((C, mode), name, st.flat.grads[name].cpu(), g32[name], GRAD_BOUND[mode]))
    cnt = st.out[1:].cpu().numpy().reshape(4, C)
    np.testing.assert_array_equal(cnt[1], np.bincount(y.ravel(), minlength=C).astype(np.float64))
    top2 = torch.topk(ref, 2, dim=1).values
    close = int(((top2[:, 0] - top2[:, 1]) < 2e-3).sum())
    pred = ref.argmax(1).numpy()
    assert cnt[2].sum() == Bn * Nn
    assert np.abs(cnt[2] - np.bincount(pred.ravel(), minlength=C)).sum() <= 2 * close
    assert np.abs(cnt[0] - np.bincount(y[pred == y], minlength=C)).sum() <= close
    print(f"[wide train step] C={C} {mode}: loss {loss:.7f} vs {ref_loss:.7f}, worst relative gradient error {worst:.2e}, "
          f"{close} points with a near tie")


def test_train_step_graph_replay_equals_eager_schedule_at_40_classes():
    """test_fused_train_step_graph_replay_equals_eager_schedule's statement with the wide loss kernels in the captured step:
    same records step by step and the same weights after them, bit for bit."""
    from randlanet._train import TrainStep
    from randlanet.utils.modules import RandLANet, RandLANetSettings
    C, K, layers, Bn, Nn = NET["C"], NET["K"], NET["layers"], 2, 2048
    rs = np.random.RandomState(0)
    x = rs.uniform(0, 1, (Bn, Nn, 3)).astype(np.float32)
    y = np.floor(x[..., 2] * C).clip(0, C - 1).astype(np.int64)
    perms = [rs.permutation(Nn) for _ in range(6)]
    records, weights = {}, {}
    for mode in ("graph", "eager"):
        torch.manual_seed(0)
        net = RandLANet(RandLANetSettings(n_classes=C, n_points=Nn, n_neighbors=K, layer_sizes=layers), DEV)
        net.fc_end[2].p = 0.0
        net.train()
        step = TrainStep(net, Bn, Nn, loss="dice", lr=1e-2, use_graph=mode == "graph")
        step.set_batch(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
        step.capture()
        rec = []
        for i, p in enumerate(perms):
            if i == 3:
                step.set_batch(torch.from_numpy(x[::-1].copy()).to(DEV), torch.from_numpy(y[::-1].copy()).to(DEV))
            step.step(p)
            rec.append(step.out.clone())
        torch.cuda.synchronize()
        records[mode] = torch.stack(rec).cpu()
        weights[mode] = step.flat.param.detach().cpu().clone()
    assert bool(torch.isfinite(records["graph"]).all())
    assert torch.equal(records["graph"], records["eager"]) and torch.equal(weights["graph"], weights["eager"])


def _scene40():
    rs = np.random.RandomState(5)
    xyz = rs.uniform((0, 0, -1), (3, 3, 1), (6000, 3)).astype(np.float32)
    labels = np.floor((xyz[:, 2] + 1) / 2 * 40).clip(0, 39).astype(np.int64)
    labels[rs.uniform(size=6000) < 0.3] = -1                    # partly labelled
    return xyz, np.zeros((6000, 0), np.float32), labels


def test_train_scenes_and_evaluate_scenes_with_40_classes():
    from randlanet import AugmentationSettings, Model, RandLANetSettings, TrainingSettings
    torch.manual_seed(0)
    np.random.seed(0)
    names = [f"class {c}" for c in range(40)]
    model = Model(RandLANetSettings(n_classes=40, n_points=2048, n_neighbors=8, layer_sizes=[8, 16, 32, 32]))
    hist = []
    scene = _scene40()
    model.train_scenes([scene], [scene], TrainingSettings(epochs=2, batch_size=2, learning_rate=1e-2, early_stopping=False,
                                                          ignore_unlabelled=True),
                       AugmentationSettings(), crops_per_epoch=4, validation_crops=2, seed=3, class_names=names,
                       callbacks=[lambda e, m: hist.append(m["loss"])], pad_small_scenes=False)
    assert len(hist) == 2 and np.all(np.isfinite(hist)), hist
    res = model.evaluate_scenes([scene], names)
    ious = [v for k, v in res.items() if k.endswith(" IoU") and k != "mIoU"]
    assert len(ious) == 40 and np.all(np.isfinite(ious)) and 0.0 <= res["mIoU"] <= 1.0


def test_training_with_300_classes_is_refused_before_any_step(ops):
    from randlanet import Model, RandLANetSettings, TrainingSettings
    from randlanet._hip import HipKernelError
    model = Model(RandLANetSettings(n_classes=300, n_points=256, n_neighbors=4, layer_sizes=[16, 32]))
    rs = np.random.RandomState(0)
    data = [(rs.uniform(0, 1, (300, 3)).astype(np.float32), np.zeros((300, 0), np.float32), rs.randint(0, 300, 300))]
    n0 = ops.H.lib().rl_launch_count()
    with pytest.raises(HipKernelError, match="Model.train: n_classes=300 exceeds the 256 classes"):
        model.train(data, data, TrainingSettings(epochs=1, batch_size=1), class_names=[f"c{i}" for i in range(300)])
    assert ops.H.lib().rl_launch_count() == n0
    # inference above the bound works as before
    conf = model.predict(data[0][0], None, prepostprocess=False)
    assert conf.shape == (300, 300) and np.allclose(conf.sum(0), 1.0, atol=1e-5)
