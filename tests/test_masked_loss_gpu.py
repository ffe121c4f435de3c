"""The masked mode of the one-shot loss kernels (rl_loss_forward_masked / rl_loss_backward_masked): points labelled outside
[0, C) count nowhere, class weights weight the labelled ones.  Yardstick: the oracle's losses on the COMPACTED labelled points
in float64 (unweighted), a float64 twin of the weighted formulas (masked_inputs.weighted_twin).  Its fp32 run differs from its
fp64 run by at most 7e-7 (loss, and relative gradient) on these inputs, so the bounds of
test_loss_metrics_against_golden_and_oracle apply unchanged: loss 2e-6 * max(1, |loss|), gradient 1e-4 * max|ref| + 1e-9."""
import numpy as np
import pytest
import torch

import masked_inputs as MI

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, N = 3, 333           # ragged against the 256-row tiles and the 32-row trips
CLASSES = (2, 5, 13, 32)
_cache = {}


def _inputs(C):
    if C not in _cache:
        g = torch.Generator().manual_seed(1000 + C)
        logits = (2.0 * torch.randn((B, C, N), generator=g)).numpy()
        labels = MI.recipe_labels(B, N, C)
        ok = (labels >= 0) & (labels < C)
        counts = np.bincount(labels[ok], minlength=C)
        _cache[C] = (logits, labels, counts, {})
    return _cache[C]


def _yard(C, name, weights):
    logits, labels, _, memo = _inputs(C)
    key = (name, weights is not None)
    if key not in memo:                 # computed once, shared, never modified
        memo[key] = MI.yardstick(name, logits, labels, weights)
    return memo[key]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(ops, logits, labels, name, weights=None, masked=True):
    kind, alpha, gamma = ops.LOSS_KINDS[name]
    kw = dict(class_weights=weights, ignore_unlabelled=masked)
    out, work = ops.loss_forward(logits, labels, kind, alpha, gamma, True, **kw)
    g = ops.loss_backward(logits, labels, kind, alpha, gamma, True, work, **kw)
    return out, g


@pytest.fixture(scope="module")
def ops():
    from randlanet import _ops
    return _ops


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("name", MI.LOSS_NAMES)
def test_masked_loss_against_the_compacted_yardstick(ops, name, C, weighted):
    from oracle import loss_metrics_oracle as LM
    from randlanet.utils.losses import class_weights_from_counts
    logits_h, labels_h, counts, _ = _inputs(C)
    MI.check_recipe(labels_h, C)
    w32 = class_weights_from_counts(counts).astype(np.float32) if weighted else None
    logits, labels = _dev(logits_h), _dev(labels_h)
    wd = _dev(w32) if weighted else None
    out, g = _run(ops, logits, labels, name, wd)
    ok = (labels_h >= 0) & (labels_h < C)

    # 1. loss and gradient; exact zeros at the unlabelled points
    ref_loss, ref_grad = _yard(C, name, w32)
    loss = float(out[0])
    gh = g.cpu().numpy()
    err_l, err_g = abs(loss - ref_loss), float(np.abs(gh - ref_grad).max())
    print(f"[masked loss] {name} C={C} weighted={weighted}: loss {loss:.9f} / {ref_loss:.9f} (diff {err_l:.2e}), "
          f"gradient diff {err_g:.2e} of max {np.abs(ref_grad).max():.2e}")
    assert err_l <= 2e-6 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    assert err_g <= 1e-4 * np.abs(ref_grad).max() + 1e-9, err_g
    dead = g.permute(0, 2, 1)[~_dev(ok)]
    assert dead.numel() > 0 and torch.equal(dead, torch.zeros_like(dead))

    # 2. integer counts of the compacted points, exactly; OA and IoU from them
    cl = np.ascontiguousarray(np.transpose(logits_h, (0, 2, 1))[ok].T)          # (C, n)
    cy = labels_h[ok]
    pred = np.argmax(cl, axis=0)
    cnt = out[1:].cpu().numpy().reshape(4, C)
    inter = np.array([((pred == c) & (cy == c)).sum() for c in range(C)], np.float64)
    np.testing.assert_array_equal(cnt[0], inter)
    np.testing.assert_array_equal(cnt[1], np.bincount(cy, minlength=C).astype(np.float64))
    np.testing.assert_array_equal(cnt[2], np.bincount(pred, minlength=C).astype(np.float64))
    p64 = torch.softmax(torch.from_numpy(cl).double(), dim=0).sum(1).numpy()
    np.testing.assert_allclose(cnt[3], p64, rtol=1e-5)
    oa, pca = LM.accuracy(cl, cy)
    miou, pci = LM.iou(cl, cy)
    assert abs(cnt[0].sum() / cnt[1].sum() - oa) < 1e-7
    for c in range(C):
        union = cnt[1][c] + cnt[2][c] - cnt[0][c]
        assert abs((1.0 if union == 0 else cnt[0][c] / union) - pci[c]) < 1e-7
        assert abs((1.0 if cnt[1][c] == 0 else cnt[0][c] / cnt[1][c]) - pca[c]) < 1e-7

    # 3. WHICH out-of-range value marks a point does not matter: bit-identical record and gradient
    other = labels_h.copy()
    other[~ok] = np.where(labels_h[~ok] == -1, C + 3, -1)
    out2, g2 = _run(ops, logits, _dev(other), name, wd)
    assert torch.equal(out2, out) and torch.equal(g2, g)

    if weighted:
        # 4. the scale of the weights cancels; all-ones weights are the unweighted masked mode
        out3, _ = _run(ops, logits, labels, name, _dev(3.0 * w32))
        assert abs(float(out3[0]) - loss) <= 1e-6 * abs(loss)
        out_u, g_u = _run(ops, logits, labels, name, None)
        out_1, g_1 = _run(ops, logits, labels, name, torch.ones(C, device=DEV))
        assert torch.equal(out_1, out_u) and torch.equal(g_1, g_u)


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("name", MI.LOSS_NAMES)
def test_masked_mode_without_unlabelled_points_is_the_default_mode(ops, name, C):
    """5. every label in range: the unweighted masked mode equals the default mode bit for bit (record and gradient)."""
    logits_h = _inputs(C)[0]
    i = np.arange(B * N, dtype=np.int64)
    labels = _dev(((7 * i + i // N) % C).reshape(B, N))
    logits = _dev(logits_h)
    out_d, g_d = _run(ops, logits, labels, name, None, masked=False)
    out_m, g_m = _run(ops, logits, labels, name, None, masked=True)
    assert torch.equal(out_m, out_d) and torch.equal(g_m, g_d)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("name", MI.LOSS_NAMES)
def test_batch_without_a_labelled_point(ops, name, C, weighted):
    """6. loss 0.0, every gradient 0, nothing non-finite."""
    logits = _dev(_inputs(C)[0])
    labels = _dev(np.resize(np.asarray(MI.OUT_OF_RANGE(C), np.int64), (B, N)))
    w = torch.linspace(0.5, 2.0, C, device=DEV) if weighted else None
    out, g = _run(ops, logits, labels, name, w)
    assert float(out[0]) == 0.0
    assert bool(torch.isfinite(out).all()) and torch.equal(out[1:], torch.zeros_like(out[1:]))
    assert torch.equal(g, torch.zeros_like(g))


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("name", MI.LOSS_NAMES)
def test_new_entries_with_the_mode_off_are_the_old_entries(ops, name, C):
    """7. default mode on the shared (partly labelled) inputs: rl_loss_forward / rl_loss_backward and the new entries with flag 0
    and null weights give the same bits."""
    H = ops.H
    lib = H.lib()
    logits_h, labels_h, _, _ = _inputs(C)
    logits, labels = _dev(logits_h), _dev(labels_h)
    kind, alpha, gamma = ops.LOSS_KINDS[name]
    out_o, work_o = ops.loss_forward(logits, labels, kind, alpha, gamma, True)
    g_o = ops.loss_backward(logits, labels, kind, alpha, gamma, True, work_o)
    work = torch.empty_like(work_o)
    out = torch.empty_like(out_o)
    g = torch.empty_like(g_o)
    H.check(lib.rl_loss_forward_masked(logits.data_ptr(), labels.data_ptr(), B, C, N, kind, alpha, gamma, 1, None, 0,
                                       work.data_ptr(), out.data_ptr(), ops._st()), "rl_loss_forward_masked")
    H.check(lib.rl_loss_backward_masked(logits.data_ptr(), labels.data_ptr(), B, C, N, kind, alpha, gamma, 1, work.data_ptr(),
                                        1.0, None, 0, g.data_ptr(), ops._st()), "rl_loss_backward_masked")
    torch.cuda.synchronize()
    assert torch.equal(out, out_o) and torch.equal(g, g_o)
    # and the default mode still gives an unlabelled point the gradient p_c / (B N): the new mode is what removes it
    assert float(g_o.permute(0, 2, 1)[labels == -1].abs().max()) > 0


def test_masked_mode_is_refused_with_the_equivalence_mode(ops):
    class FakeSync:
        pass
    logits, labels = torch.zeros((1, 2, 8), device=DEV), torch.zeros((1, 8), dtype=torch.int64, device=DEV)
    with pytest.raises(ops.H.HipKernelError, match="ignore_unlabelled / class_weights together with sync"):
        ops.loss_forward(logits, labels, 0, 0.0, 0.0, True, sync=FakeSync(), ignore_unlabelled=True)
