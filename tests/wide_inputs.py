"""Shared inputs and yardsticks of the wide-class tests (test_wide_classes_*): 33 .. 256 classes.  masked_inputs.recipe_labels
marks unlabelled points with 255 among others, which is a real class at C = 256; the recipe here marks with [-1, C, C + 255, -7]."""
import numpy as np
import torch

import masked_inputs as MI

B, N = 3, 700                   # ragged against the 256-row tiles; the tile 512 .. 767 straddles clouds 0 and 1, 1280 .. 1535 clouds 1 and 2
CLASSES = (33, 40, 64, 65, 200, 256)    # first past the old limit; both sides of a 32 / 64 class tile; the maximum
MODES = ("plain", "masked", "weighted")
MARKS = lambda C: [-1, C, C + 255, -7]      # noqa: E731


def base_labels(B: int, N: int, C: int) -> np.ndarray:
    i = np.arange(B * N, dtype=np.int64)
    return ((7 * i + i // N) % C).reshape(B, N)


def recipe_labels(B: int, N: int, C: int) -> np.ndarray:
    """base_labels; every point with flat index i % 4 == 1 takes the next of MARKS(C) in turn; cloud 1 is entirely -1."""
    lab = base_labels(B, N, C).reshape(-1)
    hit = np.flatnonzero(np.arange(B * N) % 4 == 1)
    lab[hit] = np.asarray(MARKS(C), np.int64)[np.arange(hit.size) % 4]
    lab = lab.reshape(B, N)
    lab[1] = -1
    return lab


def check_recipe(lab: np.ndarray, C: int) -> None:
    """One cloud entirely unlabelled, half of the points unlabelled, every class present, every mark in use."""
    ok = (lab >= 0) & (lab < C)
    assert 0.49 < 1.0 - ok.mean() < 0.51, ok.mean()
    assert not ok[1].any() and ok[0].any() and ok[2].any()
    assert np.bincount(lab[ok], minlength=C).min() >= 1
    assert {int(v) for v in lab[~ok]} == set(MARKS(C))


_cache = {}


def inputs(C: int):
    """(logits (B, C, N) float32 = 2 * randn, recipe labels, counts of the labelled points per class) - made once, never modified."""
    if C not in _cache:
        g = torch.Generator().manual_seed(2000 + C)
        logits = (2.0 * torch.randn((B, C, N), generator=g)).numpy()
        labels = recipe_labels(B, N, C)
        ok = (labels >= 0) & (labels < C)
        _cache[C] = (logits, labels, np.bincount(labels[ok], minlength=C))
    return _cache[C]


def mode_inputs(C: int, mode: str):
    """(logits, labels, float32 class weights or None) of a mode: plain has every label in range."""
    from randlanet.utils.losses import class_weights_from_counts
    logits, labels, counts = inputs(C)
    if mode == "plain":
        return logits, base_labels(B, N, C), None
    return logits, labels, (class_weights_from_counts(counts).astype(np.float32) if mode == "weighted" else None)


def yardstick(name: str, logits: np.ndarray, labels: np.ndarray, weights=None, dtype=torch.float64):
    """masked_inputs.yardstick in `dtype`: (loss, gradient (B, C, N) with zeros at the unlabelled points) of the oracle's
    loss_by_name on the compacted labelled points, or of masked_inputs.weighted_twin with weights."""
    from oracle.loss_metrics_oracle import loss_by_name
    lg = torch.from_numpy(logits).to(dtype)
    lb = torch.from_numpy(labels)
    cl, cy, ok = MI.compact(lg, lb)
    cl.requires_grad_(True)
    loss = loss_by_name(name, cl, cy) if weights is None else MI.weighted_twin(name, cl, cy, torch.from_numpy(np.asarray(weights)).to(dtype))
    loss.backward()
    grad = torch.zeros_like(lg).permute(0, 2, 1).contiguous()
    grad[ok] = cl.grad[0].t()
    return float(loss.detach()), grad.permute(0, 2, 1).contiguous().numpy()


def tversky_twin(logits: np.ndarray, labels: np.ndarray, alpha: float, gamma: float, neglect_background: bool, dtype=torch.float64):
    """The Tversky family over every point with the background kept or neglected (masked_inputs.weighted_twin's formula with
    unit weights, which always neglects it): (loss, gradient).  An empty class (tp = sum y = 0) keeps its term."""
    lg = torch.from_numpy(logits).to(dtype).requires_grad_(True)
    C = lg.shape[1]
    p = torch.softmax(lg, dim=1).permute(1, 0, 2).reshape(C, -1)
    y = torch.nn.functional.one_hot(torch.from_numpy(labels), C).to(dtype).permute(2, 0, 1).reshape(C, -1)
    c0 = 1 if neglect_background else 0
    p, y = p[c0:], y[c0:]
    tp, fn, fp = (y * p).sum(1), (y * (1 - p)).sum(1), ((1 - y) * p).sum(1)
    ti = (tp + MI.EPS) / (tp + alpha * fn + (1 - alpha) * fp + MI.EPS)
    loss = ((1 - ti) ** gamma).mean()
    loss.backward()
    return float(loss.detach()), lg.grad.numpy()


TVERSKY = {"dice": (0.5, 1.0), "tversky": (0.7, 1.0), "focal_tversky": (0.7, 4.0 / 3.0)}


def empty_class_inputs():
    """C = 64 with labels below 32 only: classes 32 .. 63 are empty."""
    logits = inputs(64)[0]
    return logits, base_labels(B, N, 32)
