"""Euclidean clustering of labelled points into instances: the step after the voted labels of a scene (Model.predict_scene)
that turns "these points are class c" into "these are the objects, here is where each one lies" - fixed-radius connected
components per class, as PCL's EuclideanClusterExtraction or a DBSCAN with min_samples = 1 computes them; with min_samples
above 1 the density condition of DBSCAN (Ester et al., KDD 1996), so that a thread of stray points between two objects no
longer merges them.  With `normals` and `normal_angle` the components are smoothness-constrained: two neighbours are joined only if their surface normals agree, the
condition of PCL's RegionGrowing written as an edge rule, so that two walls that meet in a corner, or a table top and the
cabinet it stands against, are two objects although they touch.

This module is the numpy host twin of csrc/cluster.hip (include/rl_randlanet.h, rl_cluster_* and rl_scene_labels) and the
public euclidean_clusters.  The twin's arithmetic is the specification; the kernels equal it bit for bit:

  coordinates   converted to float32 first; every coordinate finite; 1 <= M < 2^31 - 1
  taking part   a point takes part when its label is >= 0 and not in ignore_classes; every other point gets instance -1
  edge          r = float32(radius), r2 = r * r rounded to float32.  Two points i != j that take part are joined when they
                have the same label and d2(i, j) <= r2, d2 = (dx*dx + dy*dy) + dz*dz with dx = x_i - x_j, every operation
                rounded to float32, nothing fused.  d2 is symmetric: x_j - x_i is the exact negative of x_i - x_j
  smooth edge   with normals (M, 3) - converted to float32, every entry finite, used as given: unit length is the caller's
                business, estimate_normals delivers it - and normal_angle, 0 < normal_angle < 90 degrees: cos_t =
                float32(cos(float64(normal_angle) * pi / 180)), computed once on the host and handed to the kernel as it
                is.  An edge then needs, besides the conditions above, abs((nx_i*nx_j + ny_i*ny_j) + nz_i*nz_j) >= cos_t,
                every operation rounded to float32, nothing fused, in this order.  The expression is symmetric because float
                multiplication commutes, and unsigned, so the result does not depend on which way a normal was turned
                (vertical walls without a viewpoint get arbitrary signs).  A zero normal joins nobody.  A smooth curved
                surface is still one object - the transitive closure carries it around the bend -, only a crease cuts
  curvature     with curvature (M,) float32, finite, and max_curvature (no NaN; the two go together, and need normals): a
                point whose curvature is greater than float32(max_curvature) takes no part and gets instance -1, exactly
                like an ignored class.  These are the crease points, whose estimated normal is a blend of two surfaces
  components    the transitive closure of the edges.  A component of fewer than min_points points is dropped, its points get
                -1.  The kept components are numbered 0 .. I-1 in ascending order of their smallest point index, which makes
                the answer unique whatever order the edges are found in
  density       with min_samples > 1 (an integer >= 1; 1 is everything above, the same arithmetic and the same bits):
                near(i, j)    the plain Euclidean edge: both points take part, have the same label over all 64 bits, and
                              d2 <= r2 in un-fused float32
                support(i)    the number of j with near(i, j), i itself included.  Always the plain rule, also when
                              normal_angle is given (density is a property of the sampling, not of the orientation); points
                              that take no part - label < 0, an ignored class, curvature above max_curvature - are not counted
                core(i)       i takes part and support(i) >= min_samples (support is only ever compared with min_samples: a
                              kernel may stop counting there)
                components    the transitive closure of the edges between two CORE points (the smooth edge with normals)
                border        a point that takes part, is not core and has an edge (same rule) to at least one core point
                              joins the component of exactly one of them: the one with the smallest d2, among equal d2 the
                              lowest point index.  It transmits nothing: two components that share only border points stay
                              two.  (scikit-learn's assignment depends on the visiting order; this one does not)
                noise         every other point that takes part gets instance -1
                min_points    applies to the size of a component with its border points
                numbering     kept components in ascending order of their smallest CORE point index (a border point with a
                              lower index does not change the order); statistics run over all members, core and border
  statistics    per instance: class, count, centroid - every column summed in float64 over the members in ascending point
                index, divided by the count in float64, rounded once to float32 (the rule of grid_subsample's means) -, the
                bounding box lo / hi, and with `scores` their mean by the same fixed-order rule
  cells         the edges are found through a grid of cell edge c = r * float32(1.0625) over the box of ALL points, origin
                and dims as utils/grid.py computes them.  A grid of 2^16 cells or more on an axis is refused: below that the
                two roundings of floor((p - o) / c) displace a pair by less than 2^-6 cells, and since r / c = 16/17 <
                1 - 2^-6 two points within r of each other on an axis lie at most one cell apart.  The
                result does not depend on the cells, only the refusal does
  refusals      all ValueError, made on the host before any upload: bad shapes, labels that are not integers, non-finite
                coordinates, a radius that is not positive and finite in float32 (its square included), min_points < 1,
                a min_samples that is not an integer >= 1, and
                a grid axis of 2^16 cells or more (on the device path from the dims read back); normals without
                normal_angle or the reverse, curvature without max_curvature or the reverse, either without normals, bad
                shapes or non-finite entries of them, a normal_angle outside (0, 90), a max_curvature that is NaN
  labels        scene_labels: per row of (V, C) probabilities the argmax, ties to the lowest class; the confidence is that
                entry divided by the row's sum - float64, classes in order - rounded once to float32; the label is -1 when
                the confidence is below float32(min_confidence)
"""
from collections import namedtuple

import numpy as np

from . import grid as G

_F32 = np.float32
MAX_CLUSTER_DIM = 1 << 16       # cells per axis: keeps every joined pair within one cell of each other
CELL_FACTOR = _F32(1.0625)      # c = r * 17/16 > r / (1 - 2^-6)

ClusterResult = namedtuple("ClusterResult", ["instance", "classes", "count", "centroid", "lo", "hi", "score"])

# the cells before a point's own in key order among the 27 around it, as (dz, dy, dx); the own cell comes last
_HALF = [(dz, dy, dx) for dz in (-1, 0) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) < (0, 0, 0)] + [(0, 0, 0)]
_PAIR_BLOCK = 1 << 22           # candidate pairs tested at a time


def check_inputs(xyz, labels, radius, min_points, ignore_classes, scores):
    """The refusals of euclidean_clusters, all ValueError, made on the host (before any upload).  Returns the (M, 3) float32
    coordinates, the labels as int64, r = float32(radius), min_points as int, the ignored classes as a sorted int64 array and
    the scores as float32 (or None)."""
    with np.errstate(over="ignore"):
        r = _F32(radius)
        ok = np.isfinite(r) and r > 0 and np.isfinite(r * r) and np.isfinite(r * CELL_FACTOR)
    if not ok:
        raise ValueError(f"euclidean_clusters: radius={radius!r} must be positive and finite")
    if int(min_points) != min_points or int(min_points) < 1:
        raise ValueError(f"euclidean_clusters: min_points={min_points!r} must be an integer >= 1")
    shape = tuple(np.shape(xyz))
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"euclidean_clusters: xyz has shape {shape}, expected (M, 3)")
    M = shape[0]
    if M == 0 or M >= G.MAX_POINTS:          # (before anything is converted or copied)
        raise ValueError(f"euclidean_clusters: M={M} points, outside 1 .. 2^31 - 2")
    pts = np.ascontiguousarray(np.asarray(xyz).astype(_F32))
    bad = ~np.isfinite(pts)
    if bad.any():
        i = int(np.flatnonzero(bad.any(axis=1))[0])
        raise ValueError(f"euclidean_clusters: non-finite coordinates, first at point {i}: {pts[i].tolist()}")
    labels = np.asarray(labels)
    if labels.shape != (M,) or labels.dtype.kind not in "iu":
        raise ValueError(f"euclidean_clusters: labels have shape {tuple(labels.shape)} and dtype {labels.dtype}, "
                         f"expected ({M},) integers")
    labels = np.ascontiguousarray(labels.astype(np.int64))
    ignore = np.asarray(tuple(ignore_classes) if ignore_classes is not None else (), dtype=np.int64)
    if ignore.ndim != 1:
        raise ValueError(f"euclidean_clusters: ignore_classes has shape {tuple(ignore.shape)}, expected a flat sequence")
    if scores is not None:
        scores = np.asarray(scores)
        if scores.shape != (M,):
            raise ValueError(f"euclidean_clusters: scores have shape {tuple(scores.shape)}, expected ({M},)")
        scores = np.ascontiguousarray(scores.astype(_F32))
    return pts, labels, r, int(min_points), np.unique(ignore), scores


def check_min_samples(min_samples) -> int:
    """The refusal of min_samples, a ValueError made on the host (before any upload): an integer >= 1.  Returns it as int."""
    try:
        ok = not isinstance(min_samples, bool) and int(min_samples) == min_samples and int(min_samples) >= 1
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"euclidean_clusters: min_samples={min_samples!r} must be an integer >= 1")
    return int(min_samples)


def check_smooth(M: int, normals, normal_angle, curvature=None, max_curvature=None):
    """The refusals of the smooth rule's arguments for a cloud of M points, all ValueError, made on the host (before any
    upload).  Returns None when none of the four is given, else (normals (M, 3) float32, cos_t float32, curvature (M,) float32
    or None, float32(max_curvature) or None)."""
    if normals is None and normal_angle is None:
        if curvature is not None or max_curvature is not None:
            raise ValueError("euclidean_clusters: curvature and max_curvature need normals and normal_angle")
        return None
    if normals is None or normal_angle is None:
        raise ValueError("euclidean_clusters: normals and normal_angle go together")
    if (curvature is None) != (max_curvature is None):
        raise ValueError("euclidean_clusters: curvature and max_curvature go together")
    try:
        angle = np.float64(normal_angle)
        ok = angle.shape == () and 0.0 < angle < 90.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"euclidean_clusters: normal_angle={normal_angle!r} must be a number of degrees in (0, 90)")
    cos_t = _F32(np.cos(angle * np.pi / 180.0))
    with np.errstate(over="ignore"):            # (an entry beyond float32 becomes infinite and is refused below)
        nrm = np.asarray(normals)
        if nrm.shape != (M, 3) or nrm.dtype.kind not in "fiu":
            raise ValueError(f"euclidean_clusters: normals have shape {tuple(nrm.shape)} and dtype {nrm.dtype}, expected "
                             f"({M}, 3) numbers")
        nrm = np.ascontiguousarray(nrm.astype(_F32))
        bad = ~np.isfinite(nrm)
        if bad.any():
            i = int(np.flatnonzero(bad.any(axis=1))[0])
            raise ValueError(f"euclidean_clusters: non-finite normals, first at point {i}: {nrm[i].tolist()}")
        if curvature is None:
            return nrm, cos_t, None, None
        try:
            top = _F32(np.float64(max_curvature))
            ok = top.shape == () and not np.isnan(top)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"euclidean_clusters: max_curvature={max_curvature!r} must be a number, not NaN")
        curv = np.asarray(curvature)
        if curv.shape != (M,) or curv.dtype.kind not in "fiu":
            raise ValueError(f"euclidean_clusters: curvature has shape {tuple(curv.shape)} and dtype {curv.dtype}, expected "
                             f"({M},) numbers")
        curv = np.ascontiguousarray(curv.astype(_F32))
        bad = ~np.isfinite(curv)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise ValueError(f"euclidean_clusters: non-finite curvature, first at point {i}: {curv[i]}")
    return nrm, cos_t, curv, top


def check_dims(dims) -> None:
    """Refuse a grid with an axis of 2^16 cells or more (dims as floats or integers)."""
    if any(float(d) >= MAX_CLUSTER_DIM for d in dims):
        raise ValueError(f"euclidean_clusters: grid dimensions {[int(min(float(d), 4e18)) for d in dims]} reach 2^16 = "
                         f"{MAX_CLUSTER_DIM} cells on an axis: the radius is too small for the scene's extent")


def cell_edge(r: np.float32) -> np.float32:
    return r * CELL_FACTOR


def cluster_geometry(xyz32: np.ndarray, c: np.float32):
    """(origin (3,) float32, dims (3,) int64) of the cells of edge c over float32 coordinates; refuses dims >= 2^16."""
    lo, hi = xyz32.min(axis=0), xyz32.max(axis=0)
    o = np.floor(lo / c) * c
    d = np.maximum(np.floor((hi - o) / c) + _F32(1), _F32(1))
    assert o.dtype == _F32 and d.dtype == _F32
    check_dims(d)
    return o, d.astype(np.int64)


def key_bits(dims) -> int:
    """Bits of dims_x*dims_y*dims_z, the key of the points that take no part (at least 1)."""
    return max(1, (int(dims[0]) * int(dims[1]) * int(dims[2])).bit_length())


def takes_part(labels: np.ndarray, ignore: np.ndarray, curvature=None, max_curvature=None) -> np.ndarray:
    part = (labels >= 0) & ~np.isin(labels, ignore)
    if curvature is not None:
        part &= ~(curvature > max_curvature)
    return part


def normals_agree(na: np.ndarray, nb: np.ndarray, cos_t: np.float32) -> np.ndarray:
    """abs((nx_a*nx_b + ny_a*ny_b) + nz_a*nz_b) >= cos_t per row of two (n, 3) float32 arrays, every operation in float32."""
    with np.errstate(over="ignore", invalid="ignore"):      # (normals are used as given: a NaN dot product joins nobody)
        dot = (na[:, 0] * nb[:, 0] + na[:, 1] * nb[:, 1]) + na[:, 2] * nb[:, 2]
        assert dot.dtype == _F32
        return np.abs(dot) >= cos_t


def _edges(pts, labels, part, r, o, dims, normals=None, cos_t=None, dense=False):
    """The joined pairs (a, b) of point indices, each pair once, through the cells.  dense: the pairs of the PLAIN rule
    instead, with (d2 float32, agree bool) per pair behind them - agree: the pair is an edge under the rule asked for (all
    True without normals)."""
    r2 = r * r
    P = np.flatnonzero(part)
    if P.size == 0:
        none = (np.empty(0, np.int64), np.empty(0, np.int64))
        return none + (np.empty(0, _F32), np.empty(0, bool)) if dense else none
    out_d, out_g = [], []
    c = cell_edge(r)
    v = np.maximum(np.floor((pts[P] - o) / c), _F32(0)).astype(np.int64)
    key = (v[:, 2] * dims[1] + v[:, 1]) * dims[0] + v[:, 0]
    order = np.argsort(key, kind="stable")
    ks, ps, vs = key[order], P[order], v[order]
    out_a, out_b = [], []
    for dz, dy, dx in _HALF:
        w = vs + np.array([dx, dy, dz], np.int64)
        ok = ((w >= 0) & (w < dims)).all(axis=1)
        nk = (w[:, 2] * dims[1] + w[:, 1]) * dims[0] + w[:, 0]
        b0 = np.searchsorted(ks, nk, side="left")
        b1 = np.searchsorted(ks, nk, side="right")
        if (dz, dy, dx) == (0, 0, 0):
            b1 = np.arange(ks.size)                      # the own cell: the points before the own position
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
            ia, ib = ps[a], ps[b]
            d = pts[ia] - pts[ib]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            assert d2.dtype == _F32
            keep = (d2 <= r2) & (labels[ia] == labels[ib])
            if dense:
                ia, ib = ia[keep], ib[keep]
                out_d.append(d2[keep])
                out_g.append(normals_agree(normals[ia], normals[ib], cos_t) if normals is not None
                             else np.ones(ia.size, bool))
                out_a.append(ia)
                out_b.append(ib)
                s0 = s1
                continue
            if normals is not None:
                keep &= normals_agree(normals[ia], normals[ib], cos_t)
            out_a.append(ia[keep])
            out_b.append(ib[keep])
            s0 = s1
    if dense:
        if not out_a:
            return np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0, _F32), np.empty(0, bool)
        return np.concatenate(out_a), np.concatenate(out_b), np.concatenate(out_d), np.concatenate(out_g)
    if not out_a:
        return np.empty(0, np.int64), np.empty(0, np.int64)
    return np.concatenate(out_a), np.concatenate(out_b)


def _dense_roots(M: int, part, a, b, d2, agree, min_samples: int):
    """(root (M,) int64, member (M,) bool, core (M,) bool) under the density rule from the plain-rule pairs of _edges(dense=
    True): root = the smallest core index of a core point's component, for a border point that of the core point it joined."""
    support = np.bincount(a, minlength=M) + np.bincount(b, minlength=M) + 1        # every pair once; the point itself
    core = part & (support >= min_samples)
    a, b, d2 = a[agree], b[agree], d2[agree]
    both = core[a] & core[b]
    root = _roots(M, a[both], b[both])
    # a border point and the core points it has an edge to, from either end of a pair
    ab, ba = ~core[a] & core[b], core[a] & ~core[b]
    who = np.concatenate([a[ab], b[ba]])
    to = np.concatenate([b[ab], a[ba]])
    dist = np.concatenate([d2[ab], d2[ba]])
    order = np.lexsort((to, dist, who))                    # per border point: smallest d2, then the lowest core index
    who, to = who[order], to[order]
    first = np.flatnonzero(np.concatenate(([True], who[1:] != who[:-1]))) if who.size else np.empty(0, np.int64)
    member = core.copy()
    member[who[first]] = True
    root[who[first]] = root[to[first]]
    return root, member, core


def _roots(M: int, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """root (M,) int64: the smallest point index of every point's component under the edges (a, b)."""
    parent = np.arange(M, dtype=np.int64)
    while a.size:
        pa, pb = parent[a], parent[b]
        diff = pa != pb
        if not diff.any():
            break
        a, b, pa, pb = a[diff], b[diff], pa[diff], pb[diff]
        np.minimum.at(parent, np.maximum(pa, pb), np.minimum(pa, pb))     # the larger root under the smallest one it meets
        while True:                                                       # every point straight under its root again
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    return parent


def _fixed_mean(seg: np.ndarray, values: np.ndarray, n: np.ndarray) -> np.ndarray:
    # np.bincount adds the weights one by one in point order into float64 bins: the fixed order of the contract
    return (np.bincount(seg, weights=values, minlength=n.shape[0]) / n).astype(_F32)


def euclidean_clusters_host(xyz, labels, *, radius, min_points=1, ignore_classes=(0,), scores=None, normals=None,
                            normal_angle=None, curvature=None, max_curvature=None, min_samples=1) -> ClusterResult:
    """The numpy twin of the device clustering; see the module docstring for the contract.  Returns ClusterResult(instance
    (M,) int32 - the instance of every point, -1 for none -, classes (I,) int64, count (I,) int32, centroid (I, 3) float32,
    lo, hi (I, 3) float32 - the bounding boxes -, score (I,) float32 or None without scores).  normals, normal_angle,
    curvature, max_curvature: the smooth rule, as in euclidean_clusters; without them the Euclidean rule alone.  min_samples:
    the density rule, as in euclidean_clusters; 1 is the arithmetic without it."""
    pts, labels, r, min_points, ignore, scores = check_inputs(xyz, labels, radius, min_points, ignore_classes, scores)
    min_samples = check_min_samples(min_samples)
    M = pts.shape[0]
    nrm, cos_t, curv, top = check_smooth(M, normals, normal_angle, curvature, max_curvature) or (None,) * 4
    o, dims = cluster_geometry(pts, cell_edge(r))
    part = takes_part(labels, ignore, curv, top)
    if min_samples == 1:
        root, member, core = _roots(M, *_edges(pts, labels, part, r, o, dims, nrm, cos_t)), part, part
    else:
        root, member, core = _dense_roots(M, part, *_edges(pts, labels, part, r, o, dims, nrm, cos_t, dense=True),
                                          min_samples)
    size = np.bincount(root[member], minlength=M)
    kept = member & (size[root] >= min_points)
    heads = np.flatnonzero(kept & core & (root == np.arange(M)))  # ascending smallest (core) member
    number = np.full(M, -1, np.int64)
    number[heads] = np.arange(heads.size)
    instance = np.where(kept, number[root], -1).astype(np.int32)
    I = heads.size
    members = np.flatnonzero(kept)
    seg = instance[members].astype(np.int64)
    count = np.bincount(seg, minlength=I).astype(np.int32)
    n = count.astype(np.float64)
    centroid, lo, hi = np.empty((I, 3), _F32), np.empty((I, 3), _F32), np.empty((I, 3), _F32)
    by_seg = np.argsort(seg, kind="stable")
    starts = np.concatenate(([0], np.cumsum(count)[:-1])).astype(np.int64) if I else np.empty(0, np.int64)
    for k in range(3):
        col = pts[members, k]
        centroid[:, k] = _fixed_mean(seg, col, n)
        if I:
            lo[:, k] = np.minimum.reduceat(col[by_seg], starts)
            hi[:, k] = np.maximum.reduceat(col[by_seg], starts)
    score = _fixed_mean(seg, scores[members], n) if scores is not None else None
    return ClusterResult(instance, labels[heads], count, centroid, lo, hi, score)


def euclidean_clusters(xyz, labels, *, radius, min_points=1, ignore_classes=(0,), scores=None, device=None, normals=None,
                       normal_angle=None, curvature=None, max_curvature=None, min_samples=1) -> ClusterResult:
    """The instances of labelled points: the connected components of the points that take part (label >= 0 and not in
    ignore_classes) when two points of the same label within `radius` of each other are joined; components below min_points
    are dropped, the others numbered by their smallest point index; per instance class, count, centroid, bounding box and -
    with `scores` (M,) - mean score.  Runs on the GPU (csrc/cluster.hip) when `device` is a cuda device, or when it is None
    and one is available; otherwise euclidean_clusters_host.  Either way the result is numpy arrays, and the same ones bit
    for bit.  Small clouds too: euclidean_clusters(xyz, model.predict(xyz).argmax(0), radius=...).

    With `normals` (M, 3) and `normal_angle` (degrees, inside (0, 90)) two points are joined only if, besides, their normals
    lie within normal_angle of each other, whichever way each one points: a crease between two surfaces cuts, a smooth bend
    does not.  With `curvature` (M,) and `max_curvature` the points whose curvature is above it take no part (instance -1):
    the points on a crease, whose estimated normal is a blend of the two surfaces and would bridge them at a generous
    angle.  utils/normals.py's estimate_normals delivers both.  One without its partner, or curvature without normals, is a
    ValueError.

    With `min_samples` above 1 (an integer >= 1) the components are DBSCAN's: only a core point - one with at least
    min_samples points of its label within `radius`, itself included, whatever their normals - joins and transmits; a point
    that is not core but within reach of one joins the nearest such core point's component (ties to the lowest index) and
    passes nothing on, every other point gets -1.  A thread of stray points between two objects then no longer merges them.
    min_points counts a component with its border points; the numbering goes by the smallest core point."""
    import torch
    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device(device)
    if device.type != "cuda":
        return euclidean_clusters_host(xyz, labels, radius=radius, min_points=min_points, ignore_classes=ignore_classes,
                                       scores=scores, normals=normals, normal_angle=normal_angle, curvature=curvature,
                                       max_curvature=max_curvature, min_samples=min_samples)
    from .. import _ops as ops
    pts, labels, r, min_points, ignore, scores = check_inputs(xyz, labels, radius, min_points, ignore_classes, scores)
    min_samples = check_min_samples(min_samples)
    smooth = check_smooth(pts.shape[0], normals, normal_angle, curvature, max_curvature)
    with torch.cuda.device(device), torch.no_grad():
        def up(a):
            return torch.from_numpy(a).to(device) if a is not None else None
        if smooth is None:
            res = ops.euclidean_clusters(up(pts), up(labels), float(r), min_points, ignore, up(scores),
                                         min_samples=min_samples)
        else:
            nrm, cos_t, curv, top = smooth
            res = ops.smooth_clusters(up(pts), up(labels), float(r), up(nrm), float(cos_t), min_points, ignore, up(scores),
                                      up(curv), float(top) if top is not None else None, min_samples=min_samples)
        return ClusterResult(*(t.cpu().numpy() if t is not None else None for t in res))


# ------------------------------------------------------------------------------------------------ labels of a voted scene
def scene_labels(prob: np.ndarray, min_confidence: float = 0.0):
    """(labels (V,) int64, confidence (V,) float32) of (V, C) probabilities, which may be the un-normalised blended ones: the
    argmax of every row, ties to the lowest class; its entry divided by the row's float64 sum in class order, rounded once;
    label -1 where the confidence is below float32(min_confidence).  The twin of rl_scene_labels."""
    prob = np.asarray(prob)
    assert prob.ndim == 2 and prob.shape[1] >= 1 and prob.dtype == _F32, f"prob has shape {prob.shape}, dtype {prob.dtype}"
    assert not np.isnan(min_confidence), "min_confidence is not a number"
    best = np.argmax(prob, axis=1)                       # the first maximum: ties to the lowest class
    s = np.zeros(prob.shape[0], np.float64)
    for c in range(prob.shape[1]):
        s = s + prob[:, c]
    with np.errstate(invalid="ignore", divide="ignore"):
        conf = (prob[np.arange(prob.shape[0]), best].astype(np.float64) / s).astype(_F32)
        labels = np.where(conf < _F32(min_confidence), -1, best).astype(np.int64)
    return labels, conf
