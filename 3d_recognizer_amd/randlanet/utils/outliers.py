"""Statistical outlier removal of a point cloud: the isolated points a depth camera or a terrestrial scanner leaves floating
off the surfaces are dropped before anything else looks at the cloud (PCL's StatisticalOutlierRemoval, Open3D's
remove_statistical_outlier).  A point whose mean distance to its k nearest neighbours lies more than std_ratio standard
deviations above the cloud's mean of that quantity is removed.

This module is the numpy host twin of csrc/outliers.hip (include/rl_randlanet.h, rl_outliers_*) and the public
statistical_outliers / remove_statistical_outliers.  The twin's arithmetic is the specification; the kernels equal it bit for
bit:

  coordinates    converted to float32 first; every coordinate finite; k + 1 <= M < 2^31 - 1
  k              an integer, 1 <= k <= 63: the search is for k + 1 rows and RL_KNN_MAX_K is 64
  std_ratio      a finite float >= 0, used as float64
  neighbours     of point i: the k + 1 rows of the project's exact K-NN with support = query = the cloud (rl_knn_f32 /
                 rl_knn_f32_cpu): d2 in un-fused float32, ascending by (d2, index).  The point itself is at distance 0 and so
                 among them (with more than k + 1 coincident copies it may be a copy instead, also 0); only the d2 values are
                 used, so the result does not depend on which zero is the point's own
  mean distance  m_i = (sum over ranks j = 0 .. k of sqrt(float64(d2_j))) / float64(k): the sum starts at 0.0 and adds one
                 term at a time in rank order, every operation a correctly rounded float64 one, nothing fused.  Dividing by
                 k, not k + 1, is PCL's convention: the zero is searched for and skipped
  statistics     mu = S1 / float64(M) with S1 the fixed sum of m_i; sigma = sqrt(S2 / float64(M - 1)) with S2 the fixed sum
                 of (m_i - mu) * (m_i - mu) - Open3D's two-pass form.  "Fixed sum" is the order of utils/boxes.py for ONE id
                 whose members are the points 0 .. M-1 in ascending index: chunks of 1024, 64 lanes x 16 turns, the fold in
                 halves, then the chunk sums through the same two steps (boxes.fixed_sums(values[:, None], [M]))
  threshold      t = mu + float64(std_ratio) * sigma, the product, then the sum, un-fused
  mask           keep_i = (m_i <= t).  <= is PCL's rule: a cloud whose mean distances are all equal (sigma = 0) keeps every
                 point
  outputs        OutlierResult(keep (M,) bool, kept (M',) int64 - the kept points in ascending index -, slot (M,) int32 - the
                 position of a point among the kept ones, -1 for a removed one -, mean_distance (M,) float64, mean, std and
                 threshold as float64)
  refusals       all ValueError, made on the host before any upload: bad shapes, non-finite coordinates, k outside 1 .. 63,
                 a std_ratio that is negative or not finite, M < k + 1, M >= 2^31 - 1.  A threshold that comes back
                 non-finite is a ValueError too: coordinates so far apart that a float32 squared distance overflows

Not here: a radius-count filter (PCL's RadiusOutlierRemoval), and giving a removed point the vote of its nearest kept
neighbour - Model.predict_scene(outliers=...) leaves the removed points without a vote.
"""
from collections import namedtuple

import numpy as np

from . import boxes as B
from . import normals as N

_F32 = np.float32
MIN_K, MAX_K = 1, N.MAX_K - 1      # the search is for k + 1 rows, at most RL_KNN_MAX_K
MAX_POINTS = 2 ** 31 - 1

OutlierResult = namedtuple("OutlierResult", ["keep", "kept", "slot", "mean_distance", "mean", "std", "threshold"])


def check_inputs(xyz, k, std_ratio):
    """The refusals of statistical_outliers, all ValueError, made on the host (before any upload).  Returns the (M, 3) float32
    coordinates, k as int and std_ratio as float."""
    try:
        ok = not isinstance(k, (bool, str, bytes)) and int(k) == k and MIN_K <= int(k) <= MAX_K
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"statistical_outliers: k={k!r} must be an integer in {MIN_K} .. {MAX_K}")
    k = int(k)
    try:
        ratio = float(std_ratio)
    except (TypeError, ValueError):
        raise ValueError(f"statistical_outliers: std_ratio={std_ratio!r} must be a finite number >= 0") from None
    if isinstance(std_ratio, bool) or not np.isfinite(ratio) or ratio < 0.0:
        raise ValueError(f"statistical_outliers: std_ratio={std_ratio!r} must be a finite number >= 0")
    shape = tuple(np.shape(xyz))
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"statistical_outliers: xyz has shape {shape}, expected (M, 3)")
    M = shape[0]
    if M < k + 1 or M >= MAX_POINTS:         # (before anything is converted or copied)
        raise ValueError(f"statistical_outliers: M={M} points, outside k + 1 = {k + 1} .. 2^31 - 2")
    with np.errstate(over="ignore"):            # (a coordinate beyond float32 becomes infinite and is refused below)
        pts = np.ascontiguousarray(np.asarray(xyz).astype(_F32))
    bad = ~np.isfinite(pts)
    if bad.any():
        i = int(np.flatnonzero(bad.any(axis=1))[0])
        raise ValueError(f"statistical_outliers: non-finite coordinates, first at point {i}: {pts[i].tolist()}")
    return pts, k, ratio


def check_threshold(threshold: float) -> None:
    """The one refusal that needs the distances: a threshold that is not finite."""
    if not np.isfinite(threshold):
        raise ValueError(f"statistical_outliers: the threshold is {threshold}: the coordinates lie so far apart that a float32 "
                         "squared distance overflows")


def _distances(pts: np.ndarray, first: int, last: int, k1: int) -> np.ndarray:
    """(last - first, k1) float32: the squared distances of the library's host K-NN of the queries first .. last-1 in the
    whole cloud, ascending."""
    import torch
    from .. import _cpu
    t = torch.from_numpy(pts)
    _, d2 = _cpu.knn_host(t[None], t[None, first:last], k1)
    return d2[0].numpy()


def mean_distances(d2: np.ndarray, k: int) -> np.ndarray:
    """d2 (Q, k + 1) float32 in rank order -> (Q,) float64 mean distances of the contract."""
    s = np.zeros(d2.shape[0], np.float64)
    for j in range(k + 1):
        s = s + np.sqrt(d2[:, j].astype(np.float64))
    return s / np.float64(k)


def filter_host(m: np.ndarray, std_ratio: float) -> OutlierResult:
    """The statistics, the mask and the compaction of the contract from the (M,) float64 mean distances."""
    M = m.shape[0]
    count = np.array([M])
    with np.errstate(invalid="ignore", over="ignore"):      # (an overflowed distance: refused by the caller, by the threshold)
        mu = B.fixed_sums(m[:, None], count)[0, 0] / np.float64(M)
        d = m - mu
        sigma = np.sqrt(B.fixed_sums((d * d)[:, None], count)[0, 0] / np.float64(M - 1))
        t = mu + np.float64(std_ratio) * sigma
        keep = m <= t
    kept = np.flatnonzero(keep).astype(np.int64)
    slot = np.full(M, -1, np.int32)
    slot[kept] = np.arange(kept.shape[0], dtype=np.int32)
    return OutlierResult(keep, kept, slot, m, np.float64(mu), np.float64(sigma), np.float64(t))


def statistical_outliers_host(xyz, k: int = 16, std_ratio: float = 2.0) -> OutlierResult:
    """The numpy twin of the device filter; see the module docstring for the contract.  The neighbours come from the
    library's host K-NN (rl_knn_f32_cpu) in blocks of queries; a missing library raises."""
    pts, k, std_ratio = check_inputs(xyz, k, std_ratio)
    M = pts.shape[0]
    m = np.empty(M, np.float64)
    for first, last in N._blocks(M):
        m[first:last] = mean_distances(_distances(pts, first, last, k + 1), k)
    res = filter_host(m, std_ratio)
    check_threshold(res.threshold)
    return res


def statistical_outliers(xyz, k: int = 16, std_ratio: float = 2.0, device=None) -> OutlierResult:
    """Which points of a cloud (M, 3) are statistical outliers: OutlierResult(keep, kept, slot, mean_distance, mean, std,
    threshold) - see the module docstring.  Runs on the GPU (rl_knn_f32 + csrc/outliers.hip) when `device` is a cuda device,
    or when it is None and one is available; otherwise statistical_outliers_host.  Either way the result is numpy arrays, and
    the same ones bit for bit."""
    import torch
    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device(device)
    if device.type != "cuda":
        return statistical_outliers_host(xyz, k, std_ratio)
    from .. import _ops as ops
    pts, k, std_ratio = check_inputs(xyz, k, std_ratio)
    with torch.cuda.device(device), torch.no_grad():
        keep, slot, kept, m, stats = ops.statistical_outliers(torch.from_numpy(pts).to(device), k, std_ratio)
        return OutlierResult(keep.cpu().numpy(), kept.cpu().numpy(), slot.cpu().numpy(), m.cpu().numpy(),
                             np.float64(stats[0]), np.float64(stats[1]), np.float64(stats[2]))


def remove_statistical_outliers(xyz, *columns, k: int = 16, std_ratio: float = 2.0, device=None):
    """The cloud without its statistical outliers: the kept rows of xyz and of every further per-point array in `columns`
    (features, labels, instance ids: first dimension M), in their own types, then the OutlierResult.  What scans are filtered
    with before Model.train_scenes or the evaluate_* functions, which do not take `outliers`."""
    M = np.shape(xyz)[0] if np.ndim(xyz) else 0
    columns = [np.asarray(c) for c in columns]
    for j, c in enumerate(columns):
        if c.ndim < 1 or c.shape[0] != M:
            raise ValueError(f"remove_statistical_outliers: column {j} has shape {tuple(c.shape)}, expected ({M}, ...)")
    res = statistical_outliers(xyz, k, std_ratio, device)
    return (np.asarray(xyz)[res.kept],) + tuple(c[res.kept] for c in columns) + (res,)
