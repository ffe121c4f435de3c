"""The specification of the Lovasz-Softmax loss, randlanet/utils/lovasz.py (the numpy twin of csrc/lovasz.hip), against an
independent statement: Berman's formula in torch float64 under autograd (lovasz_inputs.berman) on the same probabilities.

Bounds.  Loss within 2^-24: the twin rounds every error to float32 (relative 2^-24 of an error <= 1 where [y = c] = 1, exact
where it is 0) and the coefficients of a class are non-negative and sum to at most 1.  dloss/dp within 1e-14: both sides
form the same float64 quotients of exact integers (measured 0 to 2e-17).  Against the float64 softmax of the logits the
loss is held to the project's loss bound 2e-6 * max(1, |loss|) (measured <= 9e-9)."""
import numpy as np
import pytest
import torch

import lovasz_inputs as LI


def _terms(name):
    from randlanet.utils.lovasz import class_major, lovasz_terms
    from randlanet.utils.scene import softmax_fixed
    z, y, w = LI.case(name)
    p = softmax_fixed(class_major(z))
    return p, y.reshape(-1), w, lovasz_terms(p, y.reshape(-1), w)


@pytest.mark.parametrize("name", LI.CASES)
def test_twin_against_bermans_formula(name):
    p, y, w, (loss, dp, coef) = _terms(name)
    ref_loss, ref_dp = LI.berman(torch.from_numpy(p.astype(np.float64)), torch.from_numpy(y), w)
    err_l, err_g = abs(loss - ref_loss), float(np.abs(dp - ref_dp).max())
    print(f"[lovasz twin] {name}: loss {loss:.12f} / {ref_loss:.12f} (diff {err_l:.2e}), dL/dp diff {err_g:.2e}")
    assert err_l <= 2.0 ** -24, (loss, ref_loss)
    assert err_g <= 1e-14, err_g
    assert coef.dtype == np.float32 and coef.min() >= 0.0                     # g >= 0
    C = p.shape[0]
    ok = (y >= 0) & (y < C)
    assert not coef[:, ~ok].any() and not dp[:, ~ok].any()                   # unlabelled points
    absent = np.bincount(y[ok], minlength=C) == 0
    assert not coef[absent].any() and not dp[absent].any()                   # absent classes
    if name in ("unlabelled", "zero_weight_sum"):
        loss, dz, _ = LI.twin(name)
        assert loss == 0.0 and not dz.any()


@pytest.mark.parametrize("name", LI.CASES)
def test_twin_against_the_float64_softmax_of_the_logits(name):
    from randlanet.utils.lovasz import class_major
    z, y, w = LI.case(name)
    loss = LI.twin(name)[0]
    p64 = torch.softmax(torch.from_numpy(class_major(z)).double(), dim=0)
    ref_loss, _ = LI.berman(p64, torch.from_numpy(y.reshape(-1)), w, order32=False)
    print(f"[lovasz twin] {name}: loss {loss:.12f}, from the float64 softmax {ref_loss:.12f} (diff {abs(loss - ref_loss):.2e})")
    assert abs(loss - ref_loss) <= 2e-6 * max(1.0, abs(ref_loss))


def test_the_cases_hold_what_they_are_for():
    from randlanet.utils.lovasz import class_major
    from randlanet.utils.scene import softmax_fixed
    z, y, _ = LI.case("ties13")
    p = softmax_fixed(class_major(z))
    assert p.size - np.unique(p).size > 30000                               # tied errors
    z, y, _ = LI.case("sat40")
    p = softmax_fixed(class_major(z))
    assert np.count_nonzero(p == 1.0) == 259 and np.count_nonzero(p == 0.0) == 259 * 39
    z, y, _ = LI.case("zeros2")
    assert (softmax_fixed(class_major(z)) == 0.5).all()
    # every error is 0.5: the order is the point index, so rank r holds point r - 1 for both classes
    from randlanet.utils.lovasz import jaccard_steps
    coef = LI.twin("zeros2")[2]
    for c in range(2):
        fg = y.reshape(-1) == c
        np.testing.assert_array_equal(coef[c], jaccard_steps(fg, int(fg.sum())).astype(np.float32))
    z, y, w = LI.case("mixed7")
    C = z.shape[1]
    assert abs(np.mean(y == -1) - 0.25) < 0.01 and abs(np.mean(y == C + 3) - 0.125) < 0.01 and (w == 0).sum() == 1
    assert np.bincount(LI.case("absent6")[1].ravel(), minlength=6)[3:].sum() == 0


def test_one_hot_probabilities_give_one_minus_iou():
    """For one-hot p the Lovasz extension is the set function itself: the mean over the present classes of 1 - IoU_c of
    the hard prediction."""
    from randlanet.utils.lovasz import lovasz_terms
    rs = np.random.RandomState(11)
    C, M = 6, 900
    y = rs.randint(0, 5, M)                  # class 5 absent from the labels (and sometimes predicted)
    pred = np.where(rs.uniform(size=M) < 0.6, y, rs.randint(0, C, M))
    p = np.zeros((C, M), np.float32)
    p[pred, np.arange(M)] = 1.0
    loss, _, coef = lovasz_terms(p, y)
    ious = []
    for c in range(5):
        inter, union = np.sum((pred == c) & (y == c)), np.sum((pred == c) | (y == c))
        ious.append(inter / union)
    assert abs(loss - float(np.mean(1.0 - np.array(ious)))) <= 1e-12
    assert coef.min() >= 0.0


def test_the_sum_with_cross_entropy():
    from randlanet.utils.lovasz import lovasz_cross_entropy_host, masked_cross_entropy_host
    z, y, w = LI.case("mixed7")
    C = z.shape[1]
    loss, grad = lovasz_cross_entropy_host(z, y, w)
    lt = torch.from_numpy(z).double().requires_grad_(True)
    yt = torch.from_numpy(np.where((y >= 0) & (y < C), y, -100))
    ce = torch.nn.functional.cross_entropy(lt, yt, weight=torch.from_numpy(w).double(), ignore_index=-100)
    ce.backward()
    l0, g0 = masked_cross_entropy_host(z, y, w.astype(np.float64))
    assert abs(l0 - float(ce.detach())) <= 1e-12 and np.abs(g0 - lt.grad.numpy()).max() <= 1e-15
    l1, g1, _ = LI.twin("mixed7")
    assert loss == l1 + l0 and np.array_equal(grad, g1 + g0)


# ------------------------------------------------------------------------------------------------------------- host surface
def test_names_and_modules():
    from randlanet import _ops as ops
    from randlanet.utils import losses as L
    assert ops.LOSS_KINDS["lovasz"] == (3, 0, 0) and ops.LOSS_KINDS["lovasz_cross_entropy"] == (4, 0, 0)
    a, b = L.get_loss("lovasz"), L.get_loss("lovasz_cross_entropy", class_weights=[1.0, 0.0, 2.0])
    assert isinstance(a, L.LovaszSoftmaxLoss) and isinstance(b, torch.nn.Module)
    assert not a._with_cross_entropy and b._with_cross_entropy
    assert a._class_weights is None and b._class_weights.tolist() == [1.0, 0.0, 2.0]
    with pytest.raises(ValueError):
        L.get_loss("lovasz", class_weights=[0.0, 0.0])
    from randlanet._hip import HipKernelError
    with pytest.raises(HipKernelError):
        a(torch.zeros(1, 3, 4), torch.zeros(1, 4, dtype=torch.int64))      # no CPU path behind the modules


def test_workspace_bytes():
    from randlanet import _hip
    L = _hip.lib()
    f, o = L.rl_lovasz_workspace_bytes, L.rl_lovasz_coef_offset
    assert f(1, 1, 1) > 0 and f(8, 13, 40960) >= 28 * 8 * 13 * 40960
    for B, C, N in [(1, 2, 64), (3, 13, 1367), (2, 40, 2048), (8, 13, 40960), (1, 255, 65536), (4, 31, 135000)]:
        base = f(B, C, N)
        assert base > 0 and f(B + 1, C, N) >= base and f(B, C + 1, N) >= base and f(B, C, N + 1) >= base
        assert 0 < o(B, C, N) and o(B, C, N) % 256 == 0 and o(B, C, N) + 4 * B * C * N <= base
    # across the point where the chunk size starts to grow (2048 * 8192 keys)
    sizes = [f(1, 16, n) for n in range(1048576 - 3, 1048576 + 70)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert f(1, 257, 64) == -1 and o(1, 257, 64) == -1 and f(1, 256, 64) > 0
    assert f(1, 1, 2 ** 31 - 1) > 0
    assert f(2, 256, 2 ** 22) == -1 and f(2 ** 15, 2, 2 ** 15) == -1 and f(1, 2, 2 ** 30) == -1       # B*N*C >= 2^31
    assert f(1, 2, 2 ** 30 - 1) > 0
    assert f(0, 2, 64) == -1 and f(1, 0, 64) == -1 and f(1, 2, 0) == -1
