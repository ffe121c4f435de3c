"""Keypoints of a labelled, scored cloud: the step after the voted labels of a scene (Model.predict_scene, scene_labels) that
turns "these points are class c, with this confidence" into "here are the recognised points": the local maxima of the
confidence over a radius, each refined to the confidence-weighted mean of its neighbourhood.  Where euclidean_clusters
answers with objects - and merges two fingertips that touch - this answers with positions, one per peak, at least `radius`
apart inside a class.

This module is the numpy host twin of csrc/keypoints.hip (include/rl_randlanet.h, rl_keypoints_*) and the public
confidence_peaks.  The twin's arithmetic is the specification; the kernels equal it bit for bit:

  inputs        as euclidean_clusters (utils/cluster.py: coordinates converted to float32 and finite, 1 <= M < 2^31 - 1, integer
                labels, a radius that is positive and finite in float32, min_points >= 1), and scores (M,), required, converted
                to float32, every one finite and >= 0; min_score is compared as float32 and must not be NaN
  part(i)       labels[i] >= 0, not in ignore_classes, and scores[i] >= float32(min_score)
  near(i, j)    labels[i] == labels[j] over all 64 bits and the clustering's edge rule unchanged: r = float32(radius), r2 = r * r
                rounded to float32, d2 = (dx*dx + dy*dy) + dz*dz <= r2 with every operation rounded to float32, nothing fused
  support(i)    the number of j with part(j) and near(i, j), i included
  live(i)       part(i) and support(i) >= min_points.  A point that is not live takes no further part: a lone confident
                outlier neither becomes a keypoint nor suppresses the real peak beside it
  beats(j, i)   scores[j] > scores[i], or the scores are equal and j < i: a strict total order, so a plateau has one peak
  peak(i)       live(i) and no live j != i with near(i, j) and beats(j, i).  The peaks are a pure function of the input, and two
                peaks of one label lie more than r apart (the weaker would have been beaten).  Keypoints are numbered in
                ascending peak index
  members       of the keypoint with peak p: the live j with near(p, j), p included, in ascending (cell key, point index) of
                the clustering's own grid - cell edge cell_edge(r), origin, dims and key as cluster_geometry computes them.
                That is the order of the stable sort by cell, so the device meets them in it without sorting anything again
  position      in float64, every product rounded before it is added, members in that order: W = sum of score_j, S_a = sum of
                score_j * (x_j,a - x_p,a); position_a = float32(x_p,a + S_a / W), the peak's own coordinate when W == 0.  The
                differences keep the sum's rounding relative to the radius, not to the coordinates
  result        KeypointResult(index (K,) int64 - the peak's point -, classes (K,) int64, position (K, 3) float32, score (K,)
                float32 - the peak's own -, mean_score (K,) float32 = float32(W / count), count (K,) int32 - the members).
                Without a keypoint every array is empty, with these dtypes and shapes
  cells         a grid of 2^16 cells or more on an axis is refused in the clustering's words (on the device path from the dims
                read back); below that two points within r of each other lie at most one cell apart on every axis (DESIGN.md,
                section 5).  The peaks do not depend on the cells; the order of the members, hence the last bits of W and S, does
"""
from collections import namedtuple

import numpy as np

from . import cluster as K

_F32 = np.float32
_PAIR_BLOCK = 1 << 22           # candidate pairs tested at a time

KeypointResult = namedtuple("KeypointResult", ["index", "classes", "position", "score", "mean_score", "count"])

# the 27 cells around a point's own as (dz, dy, dx), in ascending key order
_AROUND = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def check_inputs(xyz, labels, scores, radius, min_score, min_points, ignore_classes):
    """The refusals of confidence_peaks, all ValueError, made on the host (before any upload): those of euclidean_clusters, in
    its words, then the scores'.  Returns (xyz (M, 3) float32, labels int64, scores float32, r float32, float32(min_score),
    min_points as int, the ignored classes as a sorted int64 array)."""
    if scores is None:
        raise ValueError("confidence_peaks: scores are required")
    pts, labels, r, min_points, ignore, scores = K.check_inputs(xyz, labels, radius, min_points, ignore_classes, scores)
    if not (np.isfinite(scores) & (scores >= 0)).all():
        i = int(np.flatnonzero(~(np.isfinite(scores) & (scores >= 0)))[0])
        raise ValueError(f"confidence_peaks: scores must be finite and non-negative, first at point {i}: {scores[i]}")
    try:
        with np.errstate(over="ignore"):
            ms = _F32(np.float64(min_score))
        ok = ms.shape == () and not np.isnan(ms)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"confidence_peaks: min_score={min_score!r} must be a number, not NaN")
    return pts, labels, scores, r, ms, min_points, ignore


def empty_result() -> KeypointResult:
    return KeypointResult(np.empty(0, np.int64), np.empty(0, np.int64), np.empty((0, 3), _F32), np.empty(0, _F32),
                          np.empty(0, _F32), np.empty(0, np.int32))


def _near_pairs(pts, labels, ps, ks, vs, dims, r2, sources, candidates):
    """Blocks (a, b) of sorted positions with near(ps[a], ps[b]), a among `sources` and b among `candidates` (boolean masks
    over the sorted positions), through the 27 cells around a's; per a, over all blocks, b ascends within a cell."""
    for dz, dy, dx in _AROUND:
        w = vs + np.array([dx, dy, dz], np.int64)
        ok = ((w >= 0) & (w < dims)).all(axis=1) & sources
        nk = (w[:, 2] * dims[1] + w[:, 1]) * dims[0] + w[:, 0]
        b0 = np.searchsorted(ks, nk, side="left")
        b1 = np.searchsorted(ks, nk, side="right")
        n = np.where(ok, b1 - b0, 0)
        src = np.flatnonzero(n)
        if src.size == 0:
            continue
        ends = np.cumsum(n[src])
        s0 = 0
        while s0 < src.size:                             # blocks of sources with about _PAIR_BLOCK candidate pairs
            base = ends[s0 - 1] if s0 else 0
            s1 = max(s0 + 1, int(np.searchsorted(ends, base + _PAIR_BLOCK, side="right")))
            s = src[s0:s1]
            cnt = n[s]
            a = np.repeat(s, cnt)
            within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            b = np.repeat(b0[s], cnt) + within
            keep = candidates[b]
            a, b = a[keep], b[keep]
            ia, ib = ps[a], ps[b]
            d = pts[ia] - pts[ib]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            assert d2.dtype == _F32
            keep = (d2 <= r2) & (labels[ia] == labels[ib])
            yield a[keep], b[keep]
            s0 = s1


def confidence_peaks_host(xyz, labels, scores, *, radius, min_score=0.0, min_points=1, ignore_classes=(0,)) -> KeypointResult:
    """The numpy twin of the device keypoints; see the module docstring for the contract."""
    pts, labels, scores, r, ms, min_points, ignore = check_inputs(xyz, labels, scores, radius, min_score, min_points,
                                                                  ignore_classes)
    c = K.cell_edge(r)
    o, dims = K.cluster_geometry(pts, c)
    part = K.takes_part(labels, ignore) & (scores >= ms)
    P = np.flatnonzero(part)
    if P.size == 0:
        return empty_result()
    r2 = r * r
    v = np.maximum(np.floor((pts[P] - o) / c), _F32(0)).astype(np.int64)
    key = (v[:, 2] * dims[1] + v[:, 1]) * dims[0] + v[:, 0]
    order = np.argsort(key, kind="stable")               # ascending (cell key, point index)
    ks, ps, vs = key[order], P[order], v[order]
    n = ps.size
    everyone = np.ones(n, bool)

    support = np.zeros(n, np.int64)
    for a, _ in _near_pairs(pts, labels, ps, ks, vs, dims, r2, everyone, everyone):
        support += np.bincount(a, minlength=n)
    live = support >= min_points

    beaten = np.zeros(n, bool)
    sc = scores[ps]
    for a, b in _near_pairs(pts, labels, ps, ks, vs, dims, r2, live, live):
        beats = (sc[b] > sc[a]) | ((sc[b] == sc[a]) & (ps[b] < ps[a]))
        beaten[a[beats]] = True
    peak = live & ~beaten
    if not peak.any():
        return empty_result()

    pairs = list(_near_pairs(pts, labels, ps, ks, vs, dims, r2, peak, live))
    a, b = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    heads = np.flatnonzero(peak)
    heads = heads[np.argsort(ps[heads], kind="stable")]                  # keypoints in ascending peak index
    number = np.full(n, -1, np.int64)
    number[heads] = np.arange(heads.size)
    k = number[a]
    by = np.lexsort((b, k))                              # per keypoint, the members in ascending sorted position
    k, a, b = k[by], a[by], b[by]
    Kn = heads.size
    count = np.bincount(k, minlength=Kn)
    s = sc[b].astype(np.float64)
    # np.bincount adds the weights one by one in array order into float64 bins: the fixed order of the contract
    W = np.bincount(k, weights=s, minlength=Kn)
    peak_xyz = pts[ps[heads]]
    position = np.empty((Kn, 3), _F32)
    for ax in range(3):
        diff = pts[ps[b], ax].astype(np.float64) - pts[ps[a], ax].astype(np.float64)
        S = np.bincount(k, weights=s * diff, minlength=Kn)
        with np.errstate(invalid="ignore", divide="ignore"):
            position[:, ax] = np.where(W == 0, peak_xyz[:, ax], (peak_xyz[:, ax].astype(np.float64) + S / W).astype(_F32))
    mean = (W / count.astype(np.float64)).astype(_F32)
    return KeypointResult(ps[heads].astype(np.int64), labels[ps[heads]], position, sc[heads], mean, count.astype(np.int32))


def confidence_peaks(xyz, labels, scores, *, radius, min_score=0.0, min_points=1, ignore_classes=(0,),
                     device=None) -> KeypointResult:
    """The keypoints of labelled, scored points: among the points that take part (label >= 0 and not in ignore_classes, score
    >= min_score) and have at least min_points such points of their label within `radius` (themselves included), those that
    no other such point of their label within `radius` beats - by a higher score, or an equal one and a lower index; per
    keypoint the peak's point, class and score, the score-weighted mean position of the neighbourhood it ruled over, that
    neighbourhood's mean score and its size.  Runs on the GPU (csrc/keypoints.hip) when `device` is a cuda device, or when it
    is None and one is available; otherwise confidence_peaks_host.  Either way the result is numpy arrays, and the same ones
    bit for bit.  From Model.predict's (C, N) confidences on a small cloud:
    confidence_peaks(xyz, *scene_labels(conf.T), radius=...)."""
    import torch
    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device(device)
    if device.type != "cuda":
        return confidence_peaks_host(xyz, labels, scores, radius=radius, min_score=min_score, min_points=min_points,
                                     ignore_classes=ignore_classes)
    from .. import _ops as ops
    pts, labels, scores, r, ms, min_points, ignore = check_inputs(xyz, labels, scores, radius, min_score, min_points,
                                                                  ignore_classes)
    with torch.cuda.device(device), torch.no_grad():
        res = ops.confidence_peaks(*(torch.from_numpy(a).to(device) for a in (pts, labels, scores)), float(r), float(ms),
                                   min_points, ignore)
        return KeypointResult(*(t.cpu().numpy() for t in res))


def annotation_keypoints(xyz, annotation, radius=None) -> np.ndarray:
    """Ground-truth keypoint positions (G, 3) float32 from a per-point annotation mask (M,) (non-zero = annotated), the form
    the annotations of a recognition data set take.  Without `radius` every annotated point is a keypoint, in ascending point
    index: the clicked points themselves.  With `radius` the keypoints are the centroids of euclidean_clusters_host over the
    mask: one per group of annotated points chained within `radius`, which serves masks that were already broadened into
    small balls around the clicked points."""
    pts = np.asarray(xyz)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"annotation_keypoints: xyz has shape {tuple(pts.shape)}, expected (M, 3)")
    mask = np.asarray(annotation)
    if mask.shape != (pts.shape[0],):
        raise ValueError(f"annotation_keypoints: annotation has shape {tuple(mask.shape)}, expected ({pts.shape[0]},)")
    mask = mask != 0
    pts = np.ascontiguousarray(pts.astype(_F32))
    if radius is None or not mask.any():
        return pts[mask]
    return K.euclidean_clusters_host(pts, mask.astype(np.int64), radius=radius, ignore_classes=(0,)).centroid
