"""Shared inputs and yardsticks of the Lovasz-Softmax tests (test_lovasz_*): the cases, the twin's result per case (computed
once, never modified) and Berman's formula in torch float64 under autograd as the independent statement."""
import os

import numpy as np
import torch

_cache = {}


def _labels(rs, B, N, C):
    return rs.randint(0, C, (B, N)).astype(np.int64)


def _make(name):
    rs = np.random.RandomState(sum(map(ord, name)))
    w = None
    if name == "rand5":                   # (C, P) = (5, 2000), two clouds
        B, C, N = 2, 5, 1000
        z, y = (2 * rs.randn(B, C, N)).astype(np.float32), _labels(rs, B, N, C)
    elif name == "rand2":                 # (2, 64): a single wavefront
        B, C, N = 1, 2, 64
        z, y = (2 * rs.randn(B, C, N)).astype(np.float32), _labels(rs, B, N, C)
    elif name == "rand13":                # B*N = 4101 points: 53313 keys over 27 chunks of 2048, classes straddle chunks and clouds
        B, C, N = 3, 13, 1367
        z, y = (2 * rs.randn(B, C, N)).astype(np.float32), _labels(rs, B, N, C)
    elif name == "ties13":                # (13, 4099), logits from four values: tens of thousands of tied errors
        B, C, N = 1, 13, 4099
        z = rs.choice(np.array([-1.0, 0.0, 0.5, 2.0], np.float32), (B, C, N))
        y = _labels(rs, B, N, C)
    elif name == "sat40":                 # (40, 777), every third point saturated: p exactly 0 or 1
        B, C, N = 1, 40, 777
        z, y = (2 * rs.randn(B, C, N)).astype(np.float32), _labels(rs, B, N, C)
        hot = rs.randint(0, C, N)
        for i in range(0, N, 3):
            z[0, hot[i], i] = 200.0
    elif name == "one":                   # (3, 1)
        B, C, N = 1, 3, 1
        z, y = rs.randn(B, C, N).astype(np.float32), np.array([[1]], np.int64)
    elif name == "absent6":               # (6, 1500), labels below 3 only: absent classes
        B, C, N = 1, 6, 1500
        z, y = (2 * rs.randn(B, C, N)).astype(np.float32), _labels(rs, B, N, 3)
    elif name == "zeros2":                # (2, 64), all logits 0: every error 0.5, the order is the point index
        B, C, N = 1, 2, 64
        z, y = np.zeros((B, C, N), np.float32), _labels(rs, B, N, C)
    elif name == "mixed7":                # (7, 3001): a quarter -1, an eighth C + 3, one zero weight
        B, C, N = 1, 7, 3001
        z, y = (2 * rs.randn(B, C, N)).astype(np.float32), _labels(rs, B, N, C)
        i = np.arange(N)
        y[0, i % 4 == 1] = -1
        y[0, i % 8 == 2] = C + 3
        w = np.array([1.5, 0.25, 0.0, 2.0, 1.0, 0.5, 3.0], np.float32)
    elif name == "zero_weight_sum":       # the only present classes carry weight 0: loss 0, gradient 0
        B, C, N = 1, 4, 300
        z, y = (2 * rs.randn(B, C, N)).astype(np.float32), _labels(rs, B, N, 2)
        w = np.array([0.0, 0.0, 1.0, 2.0], np.float32)
    elif name == "unlabelled":            # no labelled point: loss 0, gradient 0
        B, C, N = 2, 4, 150
        z, y = (2 * rs.randn(B, C, N)).astype(np.float32), np.full((B, N), -1, np.int64)
        y[1] = C
    elif name == "even256":               # (256, 2049): six digit passes, an even number - every other case sorts in five
        B, C, N = 1, 256, 2049
        z, y = (2 * rs.randn(B, C, N)).astype(np.float32), _labels(rs, B, N, C)
    elif name in ("golden_c2", "golden_c5"):     # the two cases of golden/loss_metrics.npz every other loss is held to
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_metrics.npz")) as g:
            z, y = g[f"{name[7:]}/logits"], g[f"{name[7:]}/labels"]
    else:
        raise KeyError(name)
    return np.ascontiguousarray(z), y, w


CASES = ("rand5", "rand2", "rand13", "ties13", "sat40", "one", "absent6", "zeros2", "mixed7", "zero_weight_sum", "unlabelled",
         "golden_c2", "golden_c5")
GPU_CASES = CASES + ("even256",)     # the kernels' cases: the pass count of the sort has both parities


def case(name):
    """(logits (B, C, N) float32, labels (B, N) int64, float32 class weights or None) - made once, never modified."""
    if name not in _cache:
        _cache[name] = _make(name)
    return _cache[name]


_twins = {}


def twin(name):
    """(loss, dlogits, coef) of lovasz_softmax_host on the case - computed once, shared, never modified."""
    from randlanet.utils.lovasz import lovasz_softmax_host
    if name not in _twins:
        _twins[name] = lovasz_softmax_host(*case(name))
    return _twins[name]


def berman(p64: torch.Tensor, y: torch.Tensor, weights=None, order32: bool = True):
    """Berman's Lovasz-Softmax (lovasz_softmax_flat / lovasz_grad of the paper's published formula) on float64 probabilities
    p64 (C, M), a leaf under autograd, over the labelled points (0 <= y < C) and the classes present among them, the classes'
    terms weighted: (loss, dloss/dp (C, M)).  order32: the descending stable sort runs on the errors rounded to float32 -
    the order the specification states; the errors that enter the dot product stay float64."""
    C = p64.shape[0]
    ok = (y >= 0) & (y < C)
    w = torch.ones(C, dtype=torch.float64) if weights is None else torch.from_numpy(np.asarray(weights, np.float32)).double()
    p = p64.detach().clone().requires_grad_(True)
    if not bool(ok.any()):
        return 0.0, np.zeros(tuple(p.shape))
    pl, yl = p[:, ok], y[ok]
    terms, wsum = [], 0.0
    for c in range(C):
        fg = (yl == c).double()
        if fg.sum() == 0:
            continue
        err = (fg - pl[c]).abs()
        key = err.detach().float() if order32 else err.detach()
        perm = torch.sort(key, stable=True, descending=True).indices
        fs = fg[perm]
        gts = fs.sum()
        inter = gts - fs.cumsum(0)
        union = gts + (1 - fs).cumsum(0)
        jac = 1.0 - inter / union
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        terms.append(w[c] * torch.dot(err[perm], jac))
        wsum += float(w[c])
    if not wsum > 0:
        return 0.0, np.zeros(tuple(p.shape))
    loss = torch.stack(terms).sum() / wsum
    loss.backward()
    return float(loss.detach()), p.grad.numpy()
