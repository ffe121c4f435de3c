"""Oriented bounding boxes of point sets given by integer ids: where every object of Model.predict_instances (or of an
annotation, or of a user's own segmentation) lies and how it is turned - the principal axes of its points, the extent along
them and the centre of that box - next to the axis-aligned box and the count.

This module is the numpy host twin of csrc/boxes.hip (include/rl_randlanet.h, rl_boxes_*) and the public instance_boxes.
The twin's arithmetic is the specification; the kernels equal it bit for bit:

  coordinates   converted to float32 first; every coordinate finite; 1 <= M < 2^31 - 1
  ids           (M,) integers of any width.  A negative id belongs to no box.  I = n_ids, or max(ids) + 1 when n_ids is None
                (0 boxes when every id is negative); n_ids < 1, n_ids < max(ids) + 1 and n_ids >= 2^31 - 1 are refused
  members       of id k: its points in ascending point index (the stable sort by id); n_k of them, member r = 0 .. n_k - 1
  fixed sum     every float64 sum over the members of an id runs in ONE order, which depends on n_k alone:
                  chunks   member r lies in chunk r // CHUNK of its id, CHUNK = 64 * TURNS = 1024
                  lanes    inside a chunk, position w = r % CHUNK belongs to lane w % 64; a lane starts from 0.0 and adds
                           its terms in ascending w (turn w // 64 = 0 .. TURNS - 1)
                  fold     the 64 lane sums s_0 .. s_63 are folded in halves: s_l = s_l + s_(l + h) for l < h, with
                           h = 32, 16, 8, 4, 2, 1; s_0 is the chunk's sum (a lane without a term holds 0.0)
                  chunks   the chunk sums of an id go through the same two steps once more: chunk c belongs to lane c % 64,
                           a lane starts from 0.0 and adds its chunk sums in ascending c, and the 64 lanes are folded in
                           halves
                A wavefront follows this order with coalesced loads and six shuffles, a long id is split over n_k / CHUNK
                wavefronts, and nothing depends on where the id's members lie among the others
  mean          mu_a = fixed sum of float64(p_a) / n_k
  covariance    d = float64(p) - mu; C_ab = fixed sum of d_a * d_b / n_k for the six entries (00, 01, 02, 11, 12, 22).
                Nothing is fused; every operation is a correctly rounded float64 one
  axes          normals.jacobi(C): the 6 cyclic sweeps of utils/normals.py, lam = diag(A), eigenvectors the columns of V.
                The eigenvalues in descending order, ties to the lower index (a stable sort); u, w = the columns of the
                two largest.  The rotations leave V orthonormal to a few ulps only, so the axes are made so once more, with
                dot(a, b) = (a_x*b_x + a_y*b_y) + a_z*b_z and unit(a) = a / sqrt(dot(a, a)), a true division per component:
                axis 0 = unit(u); axis 1 = unit(w - dot(axis 0, w) * axis 0); each of the two then negated when its
                component of largest magnitude (ties to the lowest index) is negative; axis 2 = unit(axis 0 x axis 1), the
                float64 cross product (y0*z1 - z0*y1, z0*x1 - x0*z1, x0*y1 - y0*x1): every box is right-handed.
                axes[k, a] is axis a (a row), eigenvalues[k, a] its lam
  extent        t_a = (d_x*axis_a,x + d_y*axis_a,y) + d_z*axis_a,z in float64 with d = float64(p) - mu; min_a, max_a over
                the members (any order gives the same bits); extent_a = max_a - min_a; h_a = (min_a + max_a) * 0.5;
                center_x = ((mu_x + axis_0,x*h_0) + axis_1,x*h_1) + axis_2,x*h_2 and likewise y, z
  rounding      center, axes, extent and eigenvalues are rounded once to float32 at the end.  lo / hi are the float32
                minima / maxima of the coordinates, count is int32
  degenerate    one member, or all members identical: C = 0, every rotation is skipped, the axes are the identity, the
                extent is 0 and the center is the point.  Two members, collinear members: rank 1 - axis 0 is the line, the
                other extents are 0 up to rounding.  Coplanar members: rank 2.  An id without members: count 0, extent,
                center and eigenvalues 0, the axes the identity, lo = +inf and hi = -inf (a min / max over nothing)
  refusals      all ValueError, made on the host before any upload: bad shapes, ids that are not integers, non-finite
                coordinates, M outside 1 .. 2^31 - 2, n_ids outside max(max(ids) + 1, 1) .. 2^31 - 2
"""
from collections import namedtuple

import numpy as np

from . import normals as N

_F32 = np.float32
LANES = 64
TURNS = 16                      # terms a lane adds per chunk
CHUNK = LANES * TURNS           # members per chunk: 1024 (BX_CHUNK of csrc/boxes.hip)
MAX_POINTS = 2 ** 31 - 1
_GROUP_BLOCK = 1 << 12          # chunks (ids) the twin sums at a time: bounds its memory whatever the ids are

BoxResult = namedtuple("BoxResult", ["count", "lo", "hi", "center", "axes", "extent", "eigenvalues"])


def check_inputs(xyz, ids, n_ids):
    """The refusals of instance_boxes, all ValueError, made on the host (before any upload).  Returns the (M, 3) float32
    coordinates, the ids as a contiguous array of their own integer type (unsigned and narrow ones as int64) and I."""
    shape = tuple(np.shape(xyz))
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"instance_boxes: xyz has shape {shape}, expected (M, 3)")
    M = shape[0]
    if M == 0 or M >= MAX_POINTS:            # (before anything is converted or copied)
        raise ValueError(f"instance_boxes: M={M} points, outside 1 .. 2^31 - 2")
    ids = np.asarray(ids)
    if ids.shape != (M,) or ids.dtype.kind not in "iu":
        raise ValueError(f"instance_boxes: ids have shape {tuple(ids.shape)} and dtype {ids.dtype}, expected ({M},) integers")
    with np.errstate(over="ignore"):            # (a coordinate beyond float32 becomes infinite and is refused below)
        pts = np.ascontiguousarray(np.asarray(xyz).astype(_F32))
    bad = ~np.isfinite(pts)
    if bad.any():
        i = int(np.flatnonzero(bad.any(axis=1))[0])
        raise ValueError(f"instance_boxes: non-finite coordinates, first at point {i}: {pts[i].tolist()}")
    top = int(ids.max()) + 1
    if n_ids is None:
        I = max(top, 0)
    else:
        if isinstance(n_ids, bool) or int(n_ids) != n_ids or int(n_ids) < 1:
            raise ValueError(f"instance_boxes: n_ids={n_ids!r} must be an integer >= 1")
        I = int(n_ids)
        if I < top:
            raise ValueError(f"instance_boxes: n_ids={I} is below max(ids) + 1 = {top}")
    if I >= MAX_POINTS:
        raise ValueError(f"instance_boxes: {I} ids, outside 1 .. 2^31 - 2")
    ids = np.require(ids, requirements="CW") if ids.dtype in (np.int32, np.int64) else ids.astype(np.int64)
    return pts, ids, I


def _fold(s: np.ndarray) -> np.ndarray:
    """(..., 64) lane sums folded in halves -> (...)."""
    h = LANES // 2
    while h >= 1:
        s = s[..., :h] + s[..., h:2 * h]
        h //= 2
    return s[..., 0]


def _lane_sums(group: np.ndarray, within: np.ndarray, n_groups: int, values: np.ndarray) -> np.ndarray:
    """(n_groups, 64, E) float64: term j (values (n, E)) belongs to lane within[j] % 64 of group[j] and is added at turn
    within[j] // 64; every lane starts from 0.0 and takes its turns in ascending order."""
    acc = np.zeros((n_groups, LANES, values.shape[1]), np.float64)
    lane, turn = within % LANES, within // LANES
    top = int(turn.max()) + 1 if turn.size else 0
    if top <= 4 * TURNS:
        for t in range(top):
            m = turn == t
            acc[group[m], lane[m]] = acc[group[m], lane[m]] + values[m]       # (group, lane) occurs once per turn
    else:       # long ids: by turn through a sort instead of top passes over everything
        order = np.argsort(turn, kind="stable")
        ends = np.cumsum(np.bincount(turn, minlength=top))
        first = 0
        for t in range(top):
            m = order[first:ends[t]]
            acc[group[m], lane[m]] = acc[group[m], lane[m]] + values[m]
            first = ends[t]
    return acc


def _group_sums(values: np.ndarray, sizes: np.ndarray) -> np.ndarray:
    """values (n, E) float64 in consecutive groups of sizes (G,): per group the lane sums folded in halves, (G, E)."""
    G = sizes.shape[0]
    first = np.concatenate(([0], np.cumsum(sizes)))
    out = np.empty((G, values.shape[1]), np.float64)
    for g0 in range(0, G, _GROUP_BLOCK):
        g1 = min(G, g0 + _GROUP_BLOCK)
        a, b = int(first[g0]), int(first[g1])
        group = np.repeat(np.arange(g1 - g0), sizes[g0:g1])
        within = np.arange(a, b) - np.repeat(first[g0:g1], sizes[g0:g1])
        out[g0:g1] = _fold(_lane_sums(group, within, g1 - g0, values[a:b]).transpose(0, 2, 1))
    return out


def fixed_sums(values: np.ndarray, count: np.ndarray) -> np.ndarray:
    """The fixed-order float64 sums of the contract.  values (n, E) float64: the terms of all members, id after id in member
    order (n = count.sum()); count (I,) the members of every id.  Returns (I, E)."""
    count = count.astype(np.int64)
    chunks = (count + CHUNK - 1) // CHUNK                     # per id
    cid = np.repeat(np.arange(count.shape[0]), chunks)        # the id of every chunk
    cnum = np.arange(cid.shape[0]) - (np.cumsum(chunks) - chunks)[cid]
    sizes = np.minimum(count[cid] - cnum * CHUNK, CHUNK)      # the members of every chunk
    return _group_sums(_group_sums(values, sizes), chunks)


def axes_from_covariance(C: np.ndarray):
    """(axes (Q, 3, 3), eigenvalues (Q, 3)) in float64 - before their one rounding - from (Q, 6) covariances: Jacobi, the
    eigenvalues in descending order (ties to the lower index), the first two axes made orthonormal and sign-fixed, the third
    their normalised cross product.
    axes[q, a] is axis a."""
    lam, V = N.jacobi(C)
    Q = lam.shape[0]
    order = np.argsort(-lam, axis=1, kind="stable")
    rows = np.arange(Q)
    axes = np.empty((Q, 3, 3), np.float64)

    def unit(v):
        with np.errstate(invalid="ignore", divide="ignore"):
            return v / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])[:, None]

    def positive(v):
        big = np.argmax(np.abs(v), axis=1)                    # the first maximum: ties to the lowest index
        return np.where((v[rows, big] < 0.0)[:, None], -v, v)

    u = positive(unit(V[rows, :, order[:, 0]]))
    w = V[rows, :, order[:, 1]]
    s = (u[:, 0] * w[:, 0] + u[:, 1] * w[:, 1]) + u[:, 2] * w[:, 2]
    w = positive(unit(w - s[:, None] * u))
    axes[:, 0], axes[:, 1] = u, w
    axes[:, 2] = unit(np.stack((u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                                u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]), axis=1))
    return axes, lam[rows[:, None], order]


def moments_host(pts: np.ndarray, ids: np.ndarray, I: int):
    """(order, count (I,) int64, mean (I, 3), cov (I, 6)) of checked inputs, float64: the members of all ids, id after id in
    ascending point index, and the fixed-order mean and covariance of the contract (zeros for an id without members)."""
    key = np.where(ids >= 0, ids, I).astype(np.int64)
    order = np.argsort(key, kind="stable")
    count = np.bincount(key, minlength=I + 1)[:I].astype(np.int64)
    order = order[:int(count.sum())]
    P = pts[order].astype(np.float64)
    seg = np.repeat(np.arange(I), count)
    n = np.maximum(count, 1).astype(np.float64)[:, None]
    mean = fixed_sums(P, count) / n
    d = P - mean[seg]
    prod = np.stack((d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                     d[:, 2] * d[:, 2]), axis=1)
    cov = fixed_sums(prod, count) / n
    return order, count, mean, cov


def instance_boxes_host(xyz, ids, n_ids=None) -> BoxResult:
    """The numpy twin of the device boxes; see the module docstring for the contract.  Returns BoxResult(count (I,) int32,
    lo, hi (I, 3) - the axis-aligned box -, center (I, 3), axes (I, 3, 3) - axes[k, a] is axis a of box k -, extent (I, 3),
    eigenvalues (I, 3), all float32)."""
    pts, ids, I = check_inputs(xyz, ids, n_ids)
    order, count, mean, cov = moments_host(pts, ids, I)
    axes, lam = axes_from_covariance(cov)
    lo, hi = np.full((I, 3), np.inf, _F32), np.full((I, 3), -np.inf, _F32)
    tmin, tmax = np.zeros((I, 3), np.float64), np.zeros((I, 3), np.float64)
    full = np.flatnonzero(count)
    if full.size:
        starts = (np.cumsum(count) - count)[full]
        P32 = pts[order]
        seg = np.repeat(np.arange(I), count)
        d = P32.astype(np.float64) - mean[seg]
        A = axes[seg]
        t = (d[:, 0, None] * A[:, :, 0] + d[:, 1, None] * A[:, :, 1]) + d[:, 2, None] * A[:, :, 2]
        lo[full], hi[full] = np.minimum.reduceat(P32, starts, axis=0), np.maximum.reduceat(P32, starts, axis=0)
        tmin[full], tmax[full] = np.minimum.reduceat(t, starts, axis=0), np.maximum.reduceat(t, starts, axis=0)
    h = (tmin + tmax) * 0.5
    center = ((mean + axes[:, 0] * h[:, 0, None]) + axes[:, 1] * h[:, 1, None]) + axes[:, 2] * h[:, 2, None]
    return BoxResult(count.astype(np.int32), lo, hi, center.astype(_F32), axes.astype(_F32), (tmax - tmin).astype(_F32),
                     lam.astype(_F32))


def instance_boxes(xyz, ids, n_ids=None, device=None) -> BoxResult:
    """The oriented boxes of the point sets that the integer ids (M,) name among xyz (M, 3): per id in [0, I) the count, the
    axis-aligned box lo / hi, and center, axes (rows, right-handed, the longest first), extent and eigenvalues of the box
    along the principal axes of its points; a negative id belongs to no box, I = n_ids or max(ids) + 1.  Runs on the GPU
    (csrc/boxes.hip) when `device` is a cuda device, or when it is None and one is available; otherwise
    instance_boxes_host.  Either way the result is numpy arrays, and the same ones bit for bit."""
    import torch
    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device(device)
    if device.type != "cuda":
        return instance_boxes_host(xyz, ids, n_ids)
    from .. import _ops as ops
    pts, ids, I = check_inputs(xyz, ids, n_ids)
    with torch.cuda.device(device), torch.no_grad():
        res = ops.instance_boxes(torch.from_numpy(pts).to(device), torch.from_numpy(ids).to(device), I)
        return BoxResult(*(t.cpu().numpy() for t in res))
