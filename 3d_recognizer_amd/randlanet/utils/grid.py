"""Grid subsampling of a raw scene and whole-scene scoring: the two ends of RandLA-Net's large-scene protocol (Hu et al.,
CVPR 2020) around the voted crops of utils/scene.py.  The authors never crop raw scans: every scene first goes through
their grid_subsampling - one representative per occupied voxel: barycentre, mean features, majority label - and after voting
the sub-cloud's probabilities are carried back to every raw point, which are scored from one confusion matrix.

This module is the numpy host twin of csrc/grid.hip (include/rl_randlanet.h, rl_grid_* and rl_scene_confusion) and the public
grid_subsample.  The twin's arithmetic is the specification; the kernels equal it bit for bit:

  coordinates   converted to float32 first (as the scene code does), c = float32(cell)
  origin        o = floor(min / c) * c per axis, every operation rounded to float32
  cell          v = max(floor((p - o) / c), 0) per axis in float32 (a correctly rounded division), then an integer.  (The
                clamp matters only when o rounds to just above min; floor((p - o) / c) is then -1 for the lowest points.)
  dimensions    dims = max(floor((max - o) / c) + 1, 1) per axis
  key           (vz*dims_y + vy)*dims_x + vx as int64; output rows are the occupied cells in ascending key order
  means         every column of the (M, 3+F) cloud summed per cell in float64, the cell's points added in ascending point
                index; mean = sum / count in float64, rounded once to float32
  labels        a histogram per cell over n_classes; the most frequent class, ties to the lowest class.  With
                allow_unlabelled a label outside [0, n_classes) does not vote and a cell without a vote gets -1
"""
from collections import OrderedDict, namedtuple
from typing import List, Optional

import numpy as np

from . import metrics

_F32 = np.float32
MAX_GRID_DIM = 1 << 21          # per axis: keeps the key under 2^63
MAX_POINTS = 2 ** 31 - 1

GridResult = namedtuple("GridResult", ["xyz", "features", "labels", "inverse", "count"])


def check_inputs(xyz, features, labels, cell, n_classes, allow_unlabelled=False):
    """The refusals of grid_subsample, all ValueError, made on the host (before any upload).  Returns the (M, 3+F) float32
    cloud, the labels as int64 (or None) and c = float32(cell).  allow_unlabelled: labels outside [0, n_classes) pass."""
    c = _F32(cell)
    if not np.isfinite(c) or not c > 0:
        raise ValueError(f"grid_subsample: cell={cell!r} must be positive and finite")
    shape = tuple(np.shape(xyz))
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"grid_subsample: xyz has shape {shape}, expected (M, 3)")
    M = shape[0]
    if M == 0 or M >= MAX_POINTS:            # (before anything is converted or copied)
        raise ValueError(f"grid_subsample: M={M} points, outside 1 .. 2^31 - 2")
    cloud = np.asarray(xyz).astype(_F32)
    bad = ~np.isfinite(cloud)
    if bad.any():
        i = int(np.flatnonzero(bad.any(axis=1))[0])
        raise ValueError(f"grid_subsample: non-finite coordinates, first at point {i}: {cloud[i].tolist()}")
    if features is not None:
        features = np.asarray(features)
        if features.ndim != 2 or features.shape[0] != M:
            raise ValueError(f"grid_subsample: features have shape {tuple(features.shape)}, expected ({M}, F)")
        cloud = np.concatenate((cloud, features.astype(_F32)), axis=1)
    cloud = np.ascontiguousarray(cloud)
    if labels is not None:
        labels = np.asarray(labels)
        if labels.shape != (M,):
            raise ValueError(f"grid_subsample: labels have shape {tuple(labels.shape)}, expected ({M},)")
        if n_classes is None:
            raise ValueError("grid_subsample: labels given without n_classes")
        if int(n_classes) <= 0:
            raise ValueError(f"grid_subsample: n_classes={n_classes}")
        labels = np.ascontiguousarray(labels.astype(np.int64))
        out = (labels < 0) | (labels >= int(n_classes))
        if out.any() and not allow_unlabelled:
            i = int(np.flatnonzero(out)[0])
            raise ValueError(f"grid_subsample: label {int(labels[i])} of point {i} is outside [0, {int(n_classes)})")
    return cloud, labels, c


def check_dims(dims) -> None:
    """Refuse a grid with an axis of 2^21 cells or more (dims as floats or integers)."""
    if any(float(d) >= MAX_GRID_DIM for d in dims):
        raise ValueError(f"grid_subsample: grid dimensions {[int(min(float(d), 4e18)) for d in dims]} reach 2^21 = "
                         f"{MAX_GRID_DIM} cells on an axis: the cell is too small for the scene's extent")


def key_bits(dims) -> int:
    """Bits of the largest key dims_x*dims_y*dims_z - 1 (at least 1)."""
    total = int(dims[0]) * int(dims[1]) * int(dims[2])
    return max(1, (total - 1).bit_length())


def grid_geometry(xyz32: np.ndarray, c: np.float32):
    """(origin (3,) float32, dims (3,) int64) of float32 coordinates; refuses dims >= 2^21."""
    lo, hi = xyz32.min(axis=0), xyz32.max(axis=0)
    o = np.floor(lo / c) * c
    d = np.maximum(np.floor((hi - o) / c) + _F32(1), _F32(1))
    assert o.dtype == _F32 and d.dtype == _F32
    check_dims(d)
    return o, d.astype(np.int64)


def cell_keys(xyz32: np.ndarray, o: np.ndarray, dims: np.ndarray, c: np.float32) -> np.ndarray:
    """key (M,) int64 of every point."""
    f = np.maximum(np.floor((xyz32 - o) / c), _F32(0))
    assert f.dtype == _F32
    v = f.astype(np.int64)
    return (v[:, 2] * dims[1] + v[:, 1]) * dims[0] + v[:, 0]


def grid_subsample_host(xyz, features=None, labels=None, *, cell, n_classes=None, allow_unlabelled=False) -> GridResult:
    """The numpy twin of the device grid subsampling; see the module docstring for its arithmetic.  Returns
    GridResult(xyz (V,3) f32, features (V,F) f32 or None, labels (V,) int64 or None, inverse (M,) int32 - the output row of
    every input point -, count (V,) int32).  allow_unlabelled: labels outside [0, n_classes) are not refused; they do not
    vote, and a cell without a labelled point gets the label -1."""
    cloud, labels, c = check_inputs(xyz, features, labels, cell, n_classes, allow_unlabelled)
    M, dim = cloud.shape
    o, dims = grid_geometry(cloud[:, :3], c)
    key = cell_keys(cloud[:, :3], o, dims, c)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    head = np.empty(M, bool)
    head[0] = True
    np.not_equal(ks[1:], ks[:-1], out=head[1:])
    seg = np.cumsum(head) - 1
    V = int(seg[-1]) + 1
    inverse = np.empty(M, np.int32)
    inverse[order] = seg
    count = np.bincount(inverse, minlength=V).astype(np.int32)
    mean = np.empty((V, dim), _F32)
    n = count.astype(np.float64)
    for k in range(dim):
        # np.bincount adds the weights one by one in point order into float64 bins: the fixed order of the contract
        mean[:, k] = (np.bincount(inverse, weights=cloud[:, k], minlength=V) / n).astype(_F32)
    lab = None
    if labels is not None:
        C = int(n_classes)
        keep = (labels >= 0) & (labels < C)                     # (all of them unless allow_unlabelled)
        hist = np.bincount(inverse[keep].astype(np.int64) * C + labels[keep], minlength=V * C).reshape(V, C)
        lab = np.argmax(hist, axis=1).astype(np.int64)          # the first maximum: ties to the lowest class
        lab[hist.max(axis=1) == 0] = -1                         # no vote: unlabelled
    return GridResult(np.ascontiguousarray(mean[:, :3]), np.ascontiguousarray(mean[:, 3:]) if features is not None else None,
                      lab, inverse, count)


def grid_subsample(xyz, features=None, labels=None, *, cell, n_classes=None, device=None, allow_unlabelled=False) -> GridResult:
    """One representative per occupied voxel of edge `cell`: barycentre coordinates, mean features, the majority label
    (RandLA-Net's grid_subsampling), plus `inverse` - the representative of every input point - and `count`.  Runs on the GPU
    (csrc/grid.hip) when `device` is a cuda device, or when it is None and one is available; otherwise grid_subsample_host.
    Either way the result is numpy arrays, and the same ones bit for bit.  allow_unlabelled (partly labelled scans): labels
    outside [0, n_classes) are not refused; they do not vote, and a cell without a labelled point gets the label -1."""
    import torch
    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device(device)
    if device.type != "cuda":
        return grid_subsample_host(xyz, features, labels, cell=cell, n_classes=n_classes, allow_unlabelled=allow_unlabelled)
    from .. import _ops as ops
    cloud, labels, c = check_inputs(xyz, features, labels, cell, n_classes, allow_unlabelled)
    with torch.cuda.device(device), torch.no_grad():
        cloud_d = torch.from_numpy(cloud).to(device)
        labels_d = torch.from_numpy(labels).to(device) if labels is not None else None
        rows, lab, inverse, count = ops.grid_subsample(cloud_d, labels_d, float(c), n_classes)
        rows = rows.cpu().numpy()
        return GridResult(np.ascontiguousarray(rows[:, :3]),
                          np.ascontiguousarray(rows[:, 3:]) if features is not None else None,
                          lab.cpu().numpy() if lab is not None else None, inverse.cpu().numpy(), count.cpu().numpy())


# ------------------------------------------------------------------------------------------------ scoring a voted scene
def confusion(prob: np.ndarray, labels: np.ndarray, n_classes: int, inverse: Optional[np.ndarray] = None) -> np.ndarray:
    """(C, C) int64, row = label, column = argmax of the point's row of prob (V, C) - row inverse[i], or i - with ties to the
    lowest class.  prob may be the un-normalised blended probabilities.  Points whose label is outside [0, C) are skipped
    (unlabelled).  The twin of rl_scene_confusion."""
    C = int(n_classes)
    prob = np.asarray(prob)
    assert prob.ndim == 2 and prob.shape[1] == C, f"prob has shape {prob.shape}, expected (V, {C})"
    labels = np.asarray(labels).astype(np.int64)
    pred = np.argmax(prob, axis=1)
    if inverse is not None:
        pred = pred[np.asarray(inverse)]
    assert pred.shape == labels.shape, f"{pred.shape[0]} predictions for {labels.shape[0]} labels"
    keep = (labels >= 0) & (labels < C)
    return np.bincount(labels[keep] * C + pred[keep], minlength=C * C).reshape(C, C).astype(np.int64)


def metrics_from_confusion(conf: np.ndarray, class_names: Optional[List[str]] = None) -> OrderedDict:
    """"OA", "mAcc", "mIoU" and "<class> IoU" ("class c IoU" without names) of a confusion matrix (row = label), through
    metrics.accuracy_from_counts / iou_from_counts on (diagonal, row sums, column sums): an absent class has accuracy 1, an
    empty union IoU 1.  No "loss": none is computed over a voted scene."""
    conf = np.asarray(conf)
    assert conf.ndim == 2 and conf.shape[0] == conf.shape[1], f"confusion matrix of shape {conf.shape}"
    cnt = np.stack([np.diag(conf), conf.sum(axis=1), conf.sum(axis=0)]).astype(np.float64)
    oa, acc = metrics.accuracy_from_counts(cnt)
    miou, ious = metrics.iou_from_counts(cnt)
    d = OrderedDict([("OA", oa), ("mAcc", float(np.mean(acc))), ("mIoU", miou)])
    for c, v in enumerate(ious):
        d[(class_names[c] if class_names else f"class {c}") + " IoU"] = v
    return d
