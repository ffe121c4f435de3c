"""RANSAC plane segmentation of a point cloud: the dominant plane - the desk under a hand, the ground of an outdoor scan,
the floor and the walls of a room - is found and taken out before the clustering looks at the cloud (PCL's SACSegmentation
with SACMODEL_PLANE, Open3D's segment_plane).  T planes through three points each are scored by how many points lie within
`threshold` of them; the best one is refined by least squares over its inliers.

This module is the numpy host twin of csrc/planes.hip (include/rl_randlanet.h, rl_planes_*) and the public fit_plane /
segment_planes / remove_planes.  The twin's arithmetic is the specification; the kernels equal it bit for bit.  Everything
below is float32, one correctly rounded operation at a time and nothing fused, unless it says float64:

  coordinates    converted to float32 first; every coordinate finite; 3 <= M < 2^31 - 1
  threshold      finite and > 0, rounded once to float32
  iterations     T, an integer in 1 .. 65536 (RL_PLANES_MAX_HYPOTHESES)
  triples        (T, 3) integers in [0, M): the caller's, or np.random.default_rng(seed).integers(0, M, size=(T, 3),
                 dtype=np.int64) - a generator of its own: the global numpy stream that every forward draws its permutation
                 from is never touched.  The host draws them on both paths, so twin and device see the same hypotheses
  hypothesis t   from the points p0, p1, p2 of its triple: e1 = p1 - p0, e2 = p2 - p0;
                 c = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x), each product rounded, then the difference;
                 l2 = (cx*cx + cy*cy) + cz*cz; n = c / sqrt(l2), a correctly rounded square root and a true division per
                 component; d = -((nx*p0x + ny*p0y) + nz*p0z).  It is VALID iff l2 > 0 and l2 is finite: repeated indices,
                 coincident or collinear points and overflow are all caught by this one rule.  With `axis` (any finite
                 non-zero vector, normalised in float64 on the host and rounded to float32) it must also satisfy
                 |(nx*ax + ny*ay) + nz*az| >= cos_min, cos_min = float32(cos(radians(max_angle))), max_angle in degrees
                 inside (0, 90].  An invalid hypothesis is stored as four NaNs and so counts 0
  score          s_i = ((nx*x_i + ny*y_i) + nz*z_i) + d; point i is an inlier iff |s_i| <= threshold - <= as in PCL; a NaN
                 compares false.  counts[t] = the number of inliers, an exact integer: no summation order is involved
  best           the FIRST maximum of counts.  A maximum of 0: no plane is found - plane all NaN, inlier all False, best -1
  refinement     always, when the best count is >= 3 (otherwise the hypothesis plane is kept): mean and covariance of the
                 inliers = those of id 0 of boxes.moments_host(pts, where(inlier, 0, -1), 1) - float64, the fixed sums of
                 utils/boxes.py; the float64 normal = boxes.axes_from_covariance(cov)[0][0, 2], the axis of the smallest
                 eigenvalue, negated when its component of largest magnitude (ties to the lowest index) is negative - the
                 `positive` rule of boxes.py -, then rounded to float32: n32;
                 d = float32(-((f64(n32x)*mu_x + f64(n32y)*mu_y) + f64(n32z)*mu_z)).  The final `inlier` mask is the score
                 rule once more, with the refined plane.  The refined plane is NOT re-checked against `axis`
  outputs        PlaneFit(plane (4,) float32 [nx, ny, nz, d], inlier (M,) bool, kept (M',) int64 - the points NOT on the
                 plane in ascending index -, slot (M,) int32 - the kept row of every point, -1 for a plane point: the
                 conventions of utils/outliers.py's OutlierResult -, count - the final inliers -, best, counts (T,) int32,
                 hypotheses (T, 4) float32, centroid (3,) float64 - the inliers' mean of the refinement, NaN without one)
  peeling        segment_planes: round r fits on the M_r points that are left (compacted, in ascending index), its triples
                 from the SAME generator continued, integers(0, M_r, (T, 3)).  It stops after max_planes (1 .. 64) planes,
                 when fewer than 3 points are left, when no plane is found, and when a round's refined count is below
                 min_points - that plane is discarded and its points stay.  PlaneSegmentation(planes (P, 4) float32, counts
                 (P,) int64, plane_id (M,) int32 - -1 for none -, kept, slot)
  refusals       all ValueError, made on the host before any upload, naming the argument

Not here: predict_scenes, evaluate_* and train_* do not take remove_planes= (filter such scans with remove_planes(...));
other models (sphere, cylinder); MSAC / MLESAC scores, which are floating-point sums; adaptive early termination;
one-point hypotheses from normals; giving a removed point a vote.
"""
from collections import namedtuple
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import boxes as B

_F32 = np.float32
MAX_POINTS = 2 ** 31 - 1
MAX_HYPOTHESES = 65536              # RL_PLANES_MAX_HYPOTHESES
MAX_PLANES = 64
_BLOCK = 1 << 22                    # point-plane tests the twin holds at a time

PlaneFit = namedtuple("PlaneFit", ["plane", "inlier", "kept", "slot", "count", "best", "counts", "hypotheses", "centroid"])
PlaneSegmentation = namedtuple("PlaneSegmentation", ["planes", "counts", "plane_id", "kept", "slot"])


@dataclass(frozen=True)
class PlaneRemoval:
    """What Model.predict_scene(remove_planes=...) takes: the arguments of segment_planes."""
    threshold: float
    max_planes: int = 1
    min_points: int = 3
    iterations: int = 1024
    seed: int = 0
    axis: Optional[Tuple[float, float, float]] = None
    max_angle: Optional[float] = None


def _integer(value, lo, hi, what):
    try:
        ok = not isinstance(value, (bool, str, bytes)) and int(value) == value and lo <= int(value) <= hi
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"{what}={value!r} must be an integer in {lo} .. {hi}")
    return int(value)


def check_parameters(threshold, iterations, axis=None, max_angle=None, who="fit_plane"):
    """The refusals that do not depend on the cloud, all ValueError.  Returns (threshold as float32, T, axis (3,) float32 or
    None, cos_min as float32 (0 without an axis))."""
    try:
        thr = float(threshold)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: threshold={threshold!r} must be a finite number > 0") from None
    with np.errstate(over="ignore"):
        thr32 = _F32(thr)
    if isinstance(threshold, bool) or not np.isfinite(thr32) or not thr32 > 0:
        raise ValueError(f"{who}: threshold={threshold!r} must be a finite number > 0 in float32")
    T = _integer(iterations, 1, MAX_HYPOTHESES, f"{who}: iterations")
    if (axis is None) != (max_angle is None):
        raise ValueError(f"{who}: axis and max_angle go together, got axis={axis!r}, max_angle={max_angle!r}")
    if axis is None:
        return thr32, T, None, _F32(0.0)
    try:
        a = np.asarray(axis, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: axis={axis!r} must be three finite numbers, not all zero") from None
    if a.shape != (3,) or not np.isfinite(a).all() or not (a != 0).any():
        raise ValueError(f"{who}: axis={axis!r} must be three finite numbers, not all zero")
    a = a / np.max(np.abs(a))                       # (no overflow in the squares)
    a32 = (a / np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])).astype(_F32)
    try:
        ang = float(max_angle)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: max_angle={max_angle!r} must be degrees inside (0, 90]") from None
    if isinstance(max_angle, bool) or not 0.0 < ang <= 90.0:
        raise ValueError(f"{who}: max_angle={max_angle!r} must be degrees inside (0, 90]")
    return thr32, T, a32, _F32(np.cos(np.radians(np.float64(ang))))


def check_cloud(xyz, who="fit_plane"):
    """The refusals of the cloud, all ValueError.  Returns the (M, 3) float32 coordinates."""
    shape = tuple(np.shape(xyz))
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"{who}: xyz has shape {shape}, expected (M, 3)")
    M = shape[0]
    if M < 3 or M >= MAX_POINTS:                    # (before anything is converted or copied)
        raise ValueError(f"{who}: xyz has M={M} points, outside 3 .. 2^31 - 2")
    with np.errstate(over="ignore"):                # (a coordinate beyond float32 becomes infinite and is refused below)
        pts = np.ascontiguousarray(np.asarray(xyz).astype(_F32))
    bad = ~np.isfinite(pts)
    if bad.any():
        i = int(np.flatnonzero(bad.any(axis=1))[0])
        raise ValueError(f"{who}: xyz has non-finite coordinates, first at point {i}: {pts[i].tolist()}")
    return pts


def check_triples(triples, M, T, who="fit_plane"):
    """The caller's triples: (T, 3) integers in [0, M), as contiguous int64."""
    tri = np.asarray(triples)
    if tri.shape != (T, 3) or tri.dtype.kind not in "iu":
        raise ValueError(f"{who}: triples have shape {tuple(tri.shape)} and dtype {tri.dtype}, expected ({T}, 3) integers")
    if (tri < 0).any() or (tri >= M).any():
        raise ValueError(f"{who}: triples hold an index outside [0, {M})")
    return np.ascontiguousarray(tri.astype(np.int64))


def draw_triples(rng, M, T):
    """The T triples of one round from the fit's own generator."""
    return rng.integers(0, M, size=(T, 3), dtype=np.int64)


def check_inputs(xyz, threshold, iterations, seed, triples, axis, max_angle, who="fit_plane"):
    """Every refusal of fit_plane.  Returns (pts, threshold32, triples (T, 3) int64, axis32 or None, cos_min32)."""
    if triples is not None:
        shape = np.shape(triples)
        iterations = shape[0] if len(shape) == 2 else iterations
    thr32, T, a32, cos_min = check_parameters(threshold, iterations, axis, max_angle, who)
    pts = check_cloud(xyz, who)
    M = pts.shape[0]
    tri = draw_triples(np.random.default_rng(seed), M, T) if triples is None else check_triples(triples, M, T, who)
    return pts, thr32, tri, a32, cos_min


def hypotheses_host(pts, triples, axis32=None, cos_min=_F32(0.0)):
    """(T, 4) float32: the planes [nx, ny, nz, d] of the triples, NaN rows for the invalid ones."""
    p0, p1, p2 = pts[triples[:, 0]], pts[triples[:, 1]], pts[triples[:, 2]]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e1, e2 = p1 - p0, p2 - p0
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        l2 = (cx * cx + cy * cy) + cz * cz
        r = np.sqrt(l2)
        nx, ny, nz = cx / r, cy / r, cz / r
        d = -((nx * p0[:, 0] + ny * p0[:, 1]) + nz * p0[:, 2])
        valid = (l2 > 0) & np.isfinite(l2)
        if axis32 is not None:
            valid &= np.abs((nx * axis32[0] + ny * axis32[1]) + nz * axis32[2]) >= cos_min
    hyp = np.stack((nx, ny, nz, d), axis=1)
    assert hyp.dtype == _F32
    hyp[~valid] = np.nan
    return hyp


def inliers_host(pts, planes, thr32):
    """(P, M) bool: the score rule for every plane of planes (P, 4) float32."""
    pl = planes[:, :, None]
    with np.errstate(over="ignore", invalid="ignore"):
        s = ((pl[:, 0] * pts[None, :, 0] + pl[:, 1] * pts[None, :, 1]) + pl[:, 2] * pts[None, :, 2]) + pl[:, 3]
        assert s.dtype == _F32
        return np.abs(s) <= thr32


def counts_host(pts, hyp, thr32):
    """(T,) int32: the inliers of every hypothesis."""
    T, M = hyp.shape[0], pts.shape[0]
    counts = np.zeros(T, np.int64)
    pstep = min(M, _BLOCK)
    tstep = max(1, _BLOCK // pstep)
    for j in range(0, M, pstep):
        for t in range(0, T, tstep):
            counts[t:t + tstep] += inliers_host(pts[j:j + pstep], hyp[t:t + tstep], thr32).sum(axis=1)
    return counts.astype(np.int32)


def refined_plane(mean, cov):
    """The refinement's float64 step - sign, rounding, offset - from the inliers' mean (3,) and covariance (6,), float64:
    the (4,) float32 plane.  What the twin and the device path both call."""
    n = B.axes_from_covariance(np.asarray(cov, np.float64).reshape(1, 6))[0][0, 2]
    if n[int(np.argmax(np.abs(n)))] < 0.0:          # the first maximum: ties to the lowest index
        n = -n
    n32 = n.astype(_F32)
    m = np.asarray(mean, np.float64).reshape(3)
    n64 = n32.astype(np.float64)
    d = -((n64[0] * m[0] + n64[1] * m[1]) + n64[2] * m[2])
    with np.errstate(over="ignore"):
        return np.array([n32[0], n32[1], n32[2], _F32(d)], _F32)


def _split(inlier):
    kept = np.flatnonzero(~inlier).astype(np.int64)
    slot = np.full(inlier.shape[0], -1, np.int32)
    slot[kept] = np.arange(kept.shape[0], dtype=np.int32)
    return kept, slot


def _fit(pts, thr32, tri, a32, cos_min) -> PlaneFit:
    M = pts.shape[0]
    hyp = hypotheses_host(pts, tri, a32, cos_min)
    counts = counts_host(pts, hyp, thr32)
    best = int(np.argmax(counts))                   # the first maximum
    centroid = np.full(3, np.nan, np.float64)
    if counts[best] == 0:
        inlier = np.zeros(M, bool)
        return PlaneFit(np.full(4, np.nan, _F32), inlier, *_split(inlier), 0, -1, counts, hyp, centroid)
    plane = hyp[best].copy()
    inlier = inliers_host(pts, plane[None], thr32)[0]
    if counts[best] >= 3:
        _, _, mean, cov = B.moments_host(pts, np.where(inlier, 0, -1), 1)
        centroid = mean[0].copy()
        plane = refined_plane(mean[0], cov[0])
        inlier = inliers_host(pts, plane[None], thr32)[0]
    return PlaneFit(plane, inlier, *_split(inlier), int(inlier.sum()), best, counts, hyp, centroid)


def fit_plane_host(xyz, threshold, iterations=1024, seed=0, triples=None, axis=None, max_angle=None) -> PlaneFit:
    """The numpy twin of the device fit; see the module docstring for the contract."""
    return _fit(*check_inputs(xyz, threshold, iterations, seed, triples, axis, max_angle))


def _cuda(device):
    import torch
    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device(device)
    return device if device.type == "cuda" else None


def fit_plane(xyz, threshold, iterations=1024, seed=0, triples=None, axis=None, max_angle=None, device=None) -> PlaneFit:
    """The dominant plane of a cloud (M, 3): PlaneFit(plane, inlier, kept, slot, count, best, counts, hypotheses, centroid) -
    see the module docstring.  Runs on the GPU (csrc/planes.hip, the refinement's moments by csrc/boxes.hip) when `device` is
    a cuda device, or when it is None and one is available; otherwise fit_plane_host.  Either way the result is numpy arrays,
    and the same ones bit for bit."""
    device = _cuda(device)
    args = check_inputs(xyz, threshold, iterations, seed, triples, axis, max_angle)
    if device is None:
        return _fit(*args)
    import torch
    from .. import _ops as ops
    pts, thr32, tri, a32, cos_min = args
    with torch.cuda.device(device), torch.no_grad():
        plane, inlier, slot, kept, count, best, counts, hyp, centroid = ops.fit_plane(
            torch.from_numpy(pts).to(device), tri, float(thr32), a32, float(cos_min))
        return PlaneFit(plane, inlier.cpu().numpy(), kept.cpu().numpy(), slot.cpu().numpy(), count, best,
                        counts.cpu().numpy(), hyp.cpu().numpy(), centroid)


def check_segmentation(threshold, max_planes, min_points, iterations, axis, max_angle, who="segment_planes"):
    """The refusals of segment_planes that do not depend on the cloud.  Returns (threshold32, max_planes, min_points, T,
    axis32 or None, cos_min32)."""
    thr32, T, a32, cos_min = check_parameters(threshold, iterations, axis, max_angle, who)
    P = _integer(max_planes, 1, MAX_PLANES, f"{who}: max_planes")
    mp = _integer(min_points, 1, MAX_POINTS - 1, f"{who}: min_points")
    return thr32, P, mp, T, a32, cos_min


def segment_planes_host(xyz, threshold, max_planes=1, min_points=3, iterations=1024, seed=0, axis=None,
                        max_angle=None) -> PlaneSegmentation:
    """The numpy twin of the device peeling; see the module docstring for the contract."""
    checked = check_segmentation(threshold, max_planes, min_points, iterations, axis, max_angle)
    return segment_checked_host(check_cloud(xyz, "segment_planes"), *checked[:4], seed, *checked[4:])


def segment_checked_host(pts, thr32, P, mp, T, seed, a32, cos_min) -> PlaneSegmentation:
    """segment_planes_host of checked arguments (check_cloud, check_segmentation)."""
    M = pts.shape[0]
    rng = np.random.default_rng(seed)
    alive = np.arange(M, dtype=np.int64)            # the points that are left, in ascending index
    plane_id = np.full(M, -1, np.int32)
    planes, counts = [], []
    while len(planes) < P and alive.shape[0] >= 3:
        fit = _fit(pts, thr32, draw_triples(rng, pts.shape[0], T), a32, cos_min)
        if fit.best < 0 or fit.count < mp:
            break
        plane_id[alive[fit.inlier]] = len(planes)
        planes.append(fit.plane)
        counts.append(fit.count)
        alive, pts = alive[fit.kept], np.ascontiguousarray(pts[fit.kept])
    slot = np.full(M, -1, np.int32)
    slot[alive] = np.arange(alive.shape[0], dtype=np.int32)
    return PlaneSegmentation(np.array(planes, _F32).reshape(-1, 4), np.array(counts, np.int64), plane_id, alive, slot)


def segment_planes(xyz, threshold, max_planes=1, min_points=3, iterations=1024, seed=0, axis=None, max_angle=None,
                   device=None) -> PlaneSegmentation:
    """Up to max_planes planes of a cloud (M, 3), peeled one after the other: PlaneSegmentation(planes, counts, plane_id, kept,
    slot) - see the module docstring.  On the GPU when `device` is a cuda device, or when it is None and one is available -
    the cloud that is left stays on the device between the rounds -; otherwise segment_planes_host.  Either way the result is
    numpy arrays, and the same ones bit for bit."""
    device = _cuda(device)
    if device is None:
        return segment_planes_host(xyz, threshold, max_planes, min_points, iterations, seed, axis, max_angle)
    import torch
    from .. import _ops as ops
    thr32, P, mp, T, a32, cos_min = check_segmentation(threshold, max_planes, min_points, iterations, axis, max_angle)
    pts = check_cloud(xyz, "segment_planes")
    with torch.cuda.device(device), torch.no_grad():
        planes, counts, plane_id, kept, slot = ops.segment_planes(torch.from_numpy(pts).to(device), float(thr32), P, mp, T,
                                                                  seed, a32, float(cos_min))
        return PlaneSegmentation(planes, counts, plane_id.cpu().numpy(), kept.cpu().numpy(), slot.cpu().numpy())


def remove_planes(xyz, *columns, threshold, max_planes=1, min_points=3, iterations=1024, seed=0, axis=None, max_angle=None,
                  device=None):
    """The cloud without its planes: the kept rows of xyz and of every further per-point array in `columns` (features,
    labels, instance ids: first dimension M), in their own types, then the PlaneSegmentation.  What scans are filtered with
    before Model.train_scenes or the evaluate_* functions, which do not take `remove_planes`."""
    M = np.shape(xyz)[0] if np.ndim(xyz) else 0
    columns = [np.asarray(c) for c in columns]
    for j, c in enumerate(columns):
        if c.ndim < 1 or c.shape[0] != M:
            raise ValueError(f"remove_planes: column {j} has shape {tuple(c.shape)}, expected ({M}, ...)")
    res = segment_planes(xyz, threshold, max_planes, min_points, iterations, seed, axis, max_angle, device)
    return (np.asarray(xyz)[res.kept],) + tuple(c[res.kept] for c in columns) + (res,)
