"""Training losses of the reference (randlanet/utils/losses.py:7-87, trainer.py:244-269) on the
fused HIP loss kernel (rl_loss_forward / rl_loss_backward): one pass over the (B,C,N) logits
for softmax + the class sums, a second pass for the gradient.  Same class names, constructor
arguments and values as the reference; there is no PyTorch implementation behind them.

Partly labelled, class-imbalanced scenes (off by default): with ignore_unlabelled a point whose label is outside [0, C) adds
nothing to the loss and has a zero gradient; class_weights (C values, which imply it) weight the labelled points - cross
entropy and focal become sum w[y_i] * term_i / sum w[y_i] (torch's cross_entropy(weight=, ignore_index=)), the Tversky family
sum_c w_c (1 - TI_c)^gamma / sum_c w_c over the classes it averages.  class_weights_from_counts is the RandLA-Net authors'
formula for them.

LovaszSoftmaxLoss ("lovasz", "lovasz_cross_entropy") has no counterpart in the reference: the sorted mIoU surrogate on
rl_lovasz_forward / rl_lovasz_backward, specified by the numpy twin utils/lovasz.py.
"""
from typing import Iterable, Optional, Sequence

import numpy as np
import torch

from .. import _hip as H
from .. import _ops as ops

eps = 1e-7  # reference losses.py:4 (compiled into the kernel as LS_EPS)


def check_trainable_classes(n_classes: int, who: str) -> None:
    """The one refusal of a class count the loss kernels do not take (rl_loss_*: 1 .. RL_MAX_CLASSES), made before the first
    step of whatever trains or evaluates with a loss.  Building a model and inference have no such bound."""
    if int(n_classes) > H.MAX_LOSS_CLASSES:
        raise H.HipKernelError(f"{who}: n_classes={int(n_classes)} exceeds the {H.MAX_LOSS_CLASSES} classes the loss and metric "
                               f"kernels of this build take (RL_MAX_CLASSES): training and evaluate() stop at "
                               f"{H.MAX_LOSS_CLASSES} classes, inference (predict*, evaluate_scenes) does not")


def check_class_weights(class_weights: Sequence[float], n_classes: Optional[int] = None, first_class: int = 0) -> np.ndarray:
    """The refusals of every class_weights argument, all ValueError, made on the host: C values, each finite and >= 0, with a
    positive sum - and a positive sum over the classes first_class .. C - 1 (the ones a Tversky loss that neglects the
    background averages).  Returns them as a float32 array."""
    w = np.asarray(class_weights, dtype=np.float64)
    if w.ndim != 1 or w.size == 0 or (n_classes is not None and w.size != int(n_classes)):
        raise ValueError(f"class_weights: expected {'C' if n_classes is None else int(n_classes)} values, got shape {w.shape}")
    if not np.isfinite(w).all():
        raise ValueError(f"class_weights: every weight must be finite, got {w.tolist()}")
    if (w < 0).any():
        raise ValueError(f"class_weights: every weight must be >= 0, got {w.tolist()}")
    w32 = w.astype(np.float32)
    if not np.isfinite(w32).all():
        raise ValueError(f"class_weights: every weight must be finite in float32, got {w.tolist()}")
    if not w32.sum(dtype=np.float64) > 0:
        raise ValueError("class_weights: the weights sum to zero")
    if first_class > 0 and not w32[first_class:].sum(dtype=np.float64) > 0:
        raise ValueError(f"class_weights: the weights of the classes from {first_class} on, which this loss averages "
                         f"(neglect_background), sum to zero")
    return w32


def class_weights_from_counts(counts) -> np.ndarray:
    """1 / (counts / counts.sum() + 0.02) as float64: the class weights of the RandLA-Net authors (Hu et al., CVPR 2020)."""
    n = np.asarray(counts, dtype=np.float64)
    if n.ndim != 1 or n.size == 0 or (n < 0).any() or not n.sum() > 0:
        raise ValueError(f"class_weights_from_counts: expected non-negative counts with a positive sum, got {n.tolist()}")
    return 1.0 / (n / n.sum() + 0.02)


def class_weights_from_labels(label_arrays: Iterable, n_classes: int) -> np.ndarray:
    """class_weights_from_counts of the labelled points of the arrays (labels outside [0, n_classes) are not counted)."""
    C = int(n_classes)
    counts = np.zeros(C, np.int64)
    for a in label_arrays:
        a = np.asarray(a).astype(np.int64).ravel()
        counts += np.bincount(a[(a >= 0) & (a < C)], minlength=C)
    return class_weights_from_counts(counts)


class _HipLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, kind, alpha, gamma, neglect_background, class_weights=None, ignore_unlabelled=False):
        if not logits.is_cuda:
            raise H.HipKernelError("losses run on the MI355X only: there is no CPU path in this build")
        lg = logits.detach().to(torch.float32).contiguous()
        lb = labels.to(lg.device, torch.int64).contiguous()
        cw = None
        if class_weights is not None:
            if lg.shape[1] != class_weights.numel():
                raise ValueError(f"class_weights: {class_weights.numel()} weights for {lg.shape[1]} classes")
            cw = class_weights.to(lg.device, torch.float32).contiguous()
        with torch.cuda.device(lg.device):
            out, work = ops.loss_forward(lg, lb, kind, alpha, gamma, neglect_background, class_weights=cw,
                                         ignore_unlabelled=ignore_unlabelled)
        ctx.save_for_backward(lg, lb, work)
        ctx.cfg = (kind, alpha, gamma, neglect_background, cw, ignore_unlabelled)
        return out[0].to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        lg, lb, work = ctx.saved_tensors
        kind, alpha, gamma, neglect, cw, ignore = ctx.cfg
        with torch.cuda.device(lg.device):
            dlogits = ops.loss_backward(lg, lb, kind, alpha, gamma, neglect, work, class_weights=cw, ignore_unlabelled=ignore)
        return dlogits * grad_out, None, None, None, None, None, None, None


class _Masked(torch.nn.Module):
    """The two options every loss shares.  The checked weights are a buffer: they follow the module to its device."""

    def _set_masked(self, class_weights, ignore_unlabelled: bool, first_class: int = 0) -> None:
        self._ignore_unlabelled = bool(ignore_unlabelled) or class_weights is not None
        w = None
        if class_weights is not None:
            if torch.is_tensor(class_weights):
                class_weights = class_weights.detach().cpu().numpy()
            w = torch.from_numpy(check_class_weights(class_weights, None, first_class))
        self.register_buffer("_class_weights", w, persistent=False)


class FocalTverskyLoss(_Masked):
    """Dice (alpha .5, gamma 1), Tversky (gamma 1) and focal Tversky loss (losses.py:37-87)."""

    def __init__(self, alpha: float = 0.7, gamma: float = 4.0 / 3.0, neglect_background: bool = True,
                 class_weights: Optional[Sequence[float]] = None, ignore_unlabelled: bool = False):
        super().__init__()
        self._alpha, self._gamma, self._neglect_background = alpha, gamma, neglect_background
        self._set_masked(class_weights, ignore_unlabelled, 1 if neglect_background else 0)

    def forward(self, logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        return _HipLoss.apply(logits, labels, 2, float(self._alpha), float(self._gamma),
                              bool(self._neglect_background), self._class_weights, self._ignore_unlabelled)


class FocalLoss(_Masked):
    """Focal loss (losses.py:7-34)."""

    def __init__(self, gamma: float = 2, class_weights: Optional[Sequence[float]] = None, ignore_unlabelled: bool = False):
        super().__init__()
        self._gamma = gamma
        self._set_masked(class_weights, ignore_unlabelled)

    def forward(self, logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        return _HipLoss.apply(logits, labels, 1, 0.0, float(self._gamma), False, self._class_weights, self._ignore_unlabelled)


class CrossEntropyLoss(_Masked):
    """Mean cross entropy over all points - what torch.nn.CrossEntropyLoss() computes for the
    reference's "cross_entropy" choice (trainer.py:251-252); with class_weights / ignore_unlabelled what
    torch.nn.CrossEntropyLoss(weight=, ignore_index=) computes, every label outside [0, C) ignored."""

    def __init__(self, class_weights: Optional[Sequence[float]] = None, ignore_unlabelled: bool = False):
        super().__init__()
        self._set_masked(class_weights, ignore_unlabelled)

    def forward(self, logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        return _HipLoss.apply(logits, labels, 0, 0.0, 0.0, False, self._class_weights, self._ignore_unlabelled)


class LovaszSoftmaxLoss(_Masked):
    """The Lovasz-Softmax loss (Berman et al., CVPR 2018; utils/lovasz.py is its specification), the mIoU surrogate: the mean
    over the classes present in the batch of the Lovasz extension of each class' Jaccard loss; with with_cross_entropy the
    plain sum of it and CrossEntropyLoss with the same options.  Points labelled outside [0, C) are always skipped - with every
    label in range that changes nothing, so ignore_unlabelled is accepted and implied - and class_weights weight the classes'
    terms (a zero weight for class 0 is this loss' neglect_background)."""

    def __init__(self, class_weights: Optional[Sequence[float]] = None, ignore_unlabelled: bool = False,
                 with_cross_entropy: bool = False):
        super().__init__()
        self._with_cross_entropy = bool(with_cross_entropy)
        self._set_masked(class_weights, ignore_unlabelled)

    def forward(self, logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        return _HipLoss.apply(logits, labels, 4 if self._with_cross_entropy else 3, 0.0, 0.0, False, self._class_weights, True)


def get_loss(loss_function: str, class_weights: Optional[Sequence[float]] = None,
             ignore_unlabelled: bool = False) -> torch.nn.Module:
    """Name -> loss module with the reference's standard parameters (trainer.py:244-269)."""
    masked = dict(class_weights=class_weights, ignore_unlabelled=ignore_unlabelled)
    if loss_function == "cross_entropy":
        return CrossEntropyLoss(**masked)
    if loss_function == "focal":
        return FocalLoss(gamma=2, **masked)
    if loss_function == "dice":
        return FocalTverskyLoss(alpha=0.5, gamma=1.0, neglect_background=True, **masked)
    if loss_function == "tversky":
        return FocalTverskyLoss(alpha=0.7, gamma=1.0, neglect_background=True, **masked)
    if loss_function == "focal_tversky":
        return FocalTverskyLoss(alpha=0.7, gamma=(4.0 / 3.0), neglect_background=True, **masked)
    if loss_function == "lovasz":
        return LovaszSoftmaxLoss(**masked)
    if loss_function == "lovasz_cross_entropy":
        return LovaszSoftmaxLoss(with_cross_entropy=True, **masked)
    raise ValueError(f"Loss function {loss_function} not known!")
