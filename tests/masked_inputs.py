"""Shared inputs and yardsticks of the masked-loss tests (test_masked_*): partly labelled batches and a float64 statement of
the weighted losses over the labelled points."""
import numpy as np
import torch
import torch.nn.functional as F

OUT_OF_RANGE = lambda C: [-1, C, 255, -7]       # noqa: E731  the unlabelled values the recipe cycles through
LOSS_NAMES = ("cross_entropy", "focal", "dice", "tversky", "focal_tversky")
EPS = 1e-7


def recipe_labels(B: int, N: int, C: int) -> np.ndarray:
    """label = (7 i + i // N) % C over the flat point index i; every point with i % 4 == 1 takes the next of
    [-1, C, 255, -7] in turn; cloud 1 is entirely -1."""
    i = np.arange(B * N, dtype=np.int64)
    lab = (7 * i + i // N) % C
    hit = np.flatnonzero(i % 4 == 1)
    lab[hit] = np.asarray(OUT_OF_RANGE(C), np.int64)[np.arange(hit.size) % 4]
    lab = lab.reshape(B, N)
    lab[1] = -1
    return lab


def check_recipe(lab: np.ndarray, C: int) -> None:
    """What the tests rely on: about half the points and one whole cloud unlabelled, every class among the labelled ones."""
    ok = (lab >= 0) & (lab < C)
    assert 0.49 < 1.0 - ok.mean() < 0.51, ok.mean()
    assert not ok[1].any() and ok[0].any() and ok[2].any()
    counts = np.bincount(lab[ok], minlength=C)
    assert counts.min() >= (10 if C == 32 else 1), counts
    assert {int(v) for v in lab[~ok]} == set(OUT_OF_RANGE(C))


def compact(logits: torch.Tensor, labels: torch.Tensor):
    """The labelled points as one (1, C, n) cloud with (1, n) labels, and their mask (B, N)."""
    C = logits.shape[1]
    ok = (labels >= 0) & (labels < C)
    lg = logits.permute(0, 2, 1)[ok].t().unsqueeze(0).contiguous()
    return lg, labels[ok].unsqueeze(0), ok


def weighted_twin(name: str, logits: torch.Tensor, labels: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """The weighted losses over the labelled points, in the dtype of `logits` (compacted (1, C, n) input):
    cross entropy / focal sum w[y_i] term_i / sum w[y_i]; Tversky family sum_{c>=1} w_c (1 - TI_c)^gamma / sum_{c>=1} w_c."""
    C = logits.shape[1]
    w = w.to(logits.dtype)
    if name == "cross_entropy":
        return F.cross_entropy(logits, labels, weight=w)
    p = F.softmax(logits, dim=1)
    y = F.one_hot(labels, C).to(p.dtype).permute(0, 2, 1)
    if name == "focal":
        fl = (-y.clamp(EPS, 1.0 - EPS) * torch.log(p.clamp(EPS, 1.0 - EPS)) * (1 - p.clamp(EPS, 1.0 - EPS)) ** 2.0).sum(1)
        wi = w[labels]
        return (wi * fl).sum() / wi.sum()
    alpha, gamma = {"dice": (0.5, 1.0), "tversky": (0.7, 1.0), "focal_tversky": (0.7, 4.0 / 3.0)}[name]
    p, y = p.permute(1, 0, 2).reshape(C, -1)[1:], y.permute(1, 0, 2).reshape(C, -1)[1:]
    tp, fn, fp = (y * p).sum(1), (y * (1 - p)).sum(1), ((1 - y) * p).sum(1)
    ti = (tp + EPS) / (tp + alpha * fn + (1 - alpha) * fp + EPS)
    return (w[1:] * (1 - ti) ** gamma).sum() / w[1:].sum()


def yardstick(name: str, logits: np.ndarray, labels: np.ndarray, weights=None):
    """(loss, gradient (B, C, N) with zeros at the unlabelled points) in float64: the oracle's loss on the compacted labelled
    points without weights, the twin above with them."""
    from oracle.loss_metrics_oracle import loss_by_name
    lg = torch.from_numpy(logits).double()
    lb = torch.from_numpy(labels)
    cl, cy, ok = compact(lg, lb)
    cl.requires_grad_(True)
    loss = loss_by_name(name, cl, cy) if weights is None else weighted_twin(name, cl, cy, torch.from_numpy(np.asarray(weights)).double())
    loss.backward()
    grad = torch.zeros_like(lg).permute(0, 2, 1).contiguous()
    grad[ok] = cl.grad[0].t()
    return float(loss.detach()), grad.permute(0, 2, 1).contiguous().numpy()


def partly_labelled_scene():
    """5000 uniform points in the unit cube, 5 classes: everything with x < 0.3 unlabelled, and a random 60 % of the rest."""
    rs = np.random.RandomState(11)
    xyz = rs.uniform(0, 1, (5000, 3))
    feats = rs.normal(size=(5000, 2)).astype(np.float32)
    labels = rs.randint(0, 5, 5000).astype(np.int64)
    unl = xyz[:, 0] < 0.3
    rest = np.flatnonzero(~unl)
    unl[rs.permutation(rest)[:int(0.6 * rest.size)]] = True
    marks = np.array([-1, 5, 255, -7], np.int64)
    labels[unl] = marks[np.arange(int(unl.sum())) % 4]
    return xyz, feats, labels
