"""The Lovasz-Softmax loss (Berman, Triki, Blaschko: "The Lovasz-Softmax loss: a tractable surrogate for the optimization of
the intersection-over-union measure in neural networks", CVPR 2018) as the numpy host twin of csrc/lovasz.hip
(include/rl_randlanet.h, rl_lovasz_*): the specification the kernels are held to.

The order of the errors of a class - and with it every rank, tie and coefficient - depends on float32 values that the
kernels reproduce bit for bit (utils/scene.softmax_fixed), on integer counts and on one fixed float64 expression per rank,
so `coef` here equals the kernels' table bit for bit; the sums are float64.

    p        = softmax_fixed per point
    labelled : 0 <= label < C; L = the labelled points in flat order b*N + i, P = |L|
    per class c with G_c = #{i in L: y_i = c} > 0 ("present"):
        e_i  = |[y_i = c] - p_ci|                      in float32
        order: descending e, ties by ascending flat point index (~bits(e) ascending as uint32, stable)
        J_r  = 1 - (G_c - cum_r) / (G_c + r - cum_r)   in float64 from exact integers, cum_r the fg among the first r; J_0 = 0
        g_r  = J_r - J_(r-1)
        L_c  = sum_r float64(e at rank r) * g_r
    loss     = sum_c w_c L_c / sum_(c present) w_c     (0, and a zero gradient, when that sum is 0 or P = 0)
    dL/dp_ci = sign(p_ci - [y_i = c]) g_rank(i) w_c / sum w     (g is a constant of the step)
"""
from typing import Tuple

import numpy as np

from .scene import softmax_fixed

_F32 = np.float32


def jaccard_steps(fg_sorted: np.ndarray, G: int) -> np.ndarray:
    """g_r (float64, r = 1 .. P) of one class from its foreground flags in sorted order; G = their sum > 0."""
    r = np.arange(1, fg_sorted.size + 1, dtype=np.int64)
    cum = np.cumsum(fg_sorted.astype(np.int64))
    J = 1.0 - (G - cum).astype(np.float64) / (G + r - cum).astype(np.float64)
    return J - np.concatenate([[0.0], J[:-1]])


def masked_cross_entropy_host(logits: np.ndarray, labels: np.ndarray, class_weights=None) -> Tuple[float, np.ndarray]:
    """The masked cross entropy (rl_loss_forward_masked, kind 0) in float64: sum w[y_i] (lse_i - z_(y_i), i) / sum w[y_i] over
    the labelled points, and its gradient (B, C, N); 0 and zeros without a labelled point."""
    z = np.asarray(logits, np.float64)
    B, C, N = z.shape
    y = np.asarray(labels).astype(np.int64)
    ok = (y >= 0) & (y < C)
    w = np.ones(C) if class_weights is None else np.asarray(class_weights, np.float64)
    yc = np.where(ok, y, 0)
    wp = np.where(ok, w[yc], 0.0)                                   # (B, N)
    W = wp.sum()
    if not W > 0:
        return 0.0, np.zeros_like(z)
    m = z.max(axis=1, keepdims=True)
    ex = np.exp(z - m)
    den = ex.sum(axis=1, keepdims=True)
    lse = (np.log(den) + m)[:, 0]
    zy = np.take_along_axis(z, yc[:, None, :], axis=1)[:, 0]
    loss = float((wp * (lse - zy)).sum() / W)
    onehot = (np.arange(C)[None, :, None] == yc[:, None, :]).astype(np.float64)
    return loss, (ex / den - onehot) * (wp / W)[:, None, :]


def lovasz_terms(p: np.ndarray, y: np.ndarray, class_weights=None) -> Tuple[float, np.ndarray, np.ndarray]:
    """(loss, dloss/dp (C, M) float64, coef (C, M) float32) of float32 probabilities p (C, M) and flat labels y (M)."""
    p = np.ascontiguousarray(p, dtype=_F32)
    C, M = p.shape
    y = np.asarray(y).astype(np.int64).reshape(M)
    w = np.ones(C, np.float64) if class_weights is None else np.asarray(class_weights, _F32).astype(np.float64)
    lab = np.flatnonzero((y >= 0) & (y < C))
    coef = np.zeros((C, M), _F32)
    dp = np.zeros((C, M), np.float64)
    G = np.bincount(y[lab], minlength=C)
    W = float(sum(w[c] for c in range(C) if G[c] > 0))
    loss = 0.0
    if lab.size:
        for c in range(C):
            if G[c] == 0:
                continue
            fg = (y[lab] == c)
            e = np.abs(fg.astype(_F32) - p[c, lab])                               # float32
            order = np.argsort(~e.view(np.uint32), kind="stable")
            g = jaccard_steps(fg[order], int(G[c]))
            loss += w[c] * float(np.sum(e[order].astype(np.float64) * g))
            gi = np.empty_like(g)
            gi[order] = g
            coef[c, lab] = gi.astype(_F32)
            if W > 0:
                dp[c, lab] = np.sign(p[c, lab].astype(np.float64) - fg) * gi * (w[c] / W)
        loss = loss / W if W > 0 else 0.0          # (the coefficients do not depend on the weights: they stay)
    return float(loss), dp, coef


def class_major(logits: np.ndarray) -> np.ndarray:
    """(B, C, N) -> (C, B*N) float32, column b*N + i."""
    z = np.ascontiguousarray(logits, dtype=_F32)
    return np.ascontiguousarray(np.transpose(z, (1, 0, 2)).reshape(z.shape[1], -1))


def lovasz_softmax_host(logits: np.ndarray, labels: np.ndarray, class_weights=None) -> Tuple[float, np.ndarray, np.ndarray]:
    """(loss, dlogits (B, C, N) float64, coef (C, B*N) float32) of float32 logits (B, C, N) and labels (B, N)."""
    B, C, N = np.shape(logits)
    p = softmax_fixed(class_major(logits))
    loss, dp, coef = lovasz_terms(p, np.asarray(labels).reshape(B * N), class_weights)
    p64 = p.astype(np.float64)
    dz = p64 * (dp - (dp * p64).sum(axis=0, keepdims=True))
    return loss, np.ascontiguousarray(np.transpose(dz.reshape(C, B, N), (1, 0, 2))), coef


def lovasz_cross_entropy_host(logits: np.ndarray, labels: np.ndarray, class_weights=None) -> Tuple[float, np.ndarray]:
    """"lovasz_cross_entropy": the plain sum, value and gradient, of lovasz_softmax_host and the masked cross entropy."""
    l1, g1, _ = lovasz_softmax_host(logits, labels, class_weights)
    w = None if class_weights is None else np.asarray(class_weights, _F32).astype(np.float64)
    l0, g0 = masked_cross_entropy_host(logits, labels, w)
    return l1 + l0, g1 + g0
