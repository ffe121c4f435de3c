"""Surface normals and curvature of a bare point cloud, estimated from every point's k nearest neighbours: the four feature
columns [n_x, n_y, n_z, curvature] that scans without colour are usually segmented with (PCL's NormalEstimation: the
eigenvector of the neighbourhood's covariance with the smallest eigenvalue, and that eigenvalue's share of the trace).

This module is the numpy host twin of csrc/normals.hip (include/rl_randlanet.h, rl_normals) and the public
estimate_normals / normal_features.  The twin's arithmetic is the specification; the kernel equals it bit for bit:

  coordinates   converted to float32 first; every coordinate finite; k <= M < 2^31 - 1
  k             an integer, 3 <= k <= 64 (RL_KNN_MAX_K)
  neighbours    of point i: the k rows of the project's exact K-NN with support = query = the cloud (rl_knn_f32 /
                rl_knn_f32_cpu): d2 in un-fused float32, ascending by (d2, index); the point itself is among them.  Rank
                order is the order of every sum below
  centroid      float64, nothing fused: mu_a = (sum over ranks j = 0 .. k-1 of p_j,a) / k, added one by one in rank order
  covariance    d_j = p_j - mu; C_ab = (sum over ranks of d_j,a * d_j,b) / k for the six entries a <= b, in the order
                (00, 01, 02, 11, 12, 22), added one by one in rank order
  eigenvectors  cyclic Jacobi, exactly 6 sweeps over the pairs (0,1), (0,2), (1,2), A = C, V = I.  A pair (p, q) with
                A_pq == 0 is skipped; otherwise theta = (A_qq - A_pp) / (2 * A_pq),
                t = (theta >= 0 ? 1 : -1) / (|theta| + sqrt(theta*theta + 1)), c = 1 / sqrt(t*t + 1), s = t * c; then, r the
                third index: A_pp -= t*A_pq, A_qq += t*A_pq, A_pq = 0, (A_rp, A_rq) = (c*A_rp - s*A_rq, s*A_rp + c*A_rq), and
                the columns p and q of V likewise: (V_ip, V_iq) = (c*V_ip - s*V_iq, s*V_ip + c*V_iq).  Only + - * / sqrt,
                each one correctly rounded in float64
  outputs       lam = diag(A); i0 = the index of the smallest lam, ties to the lowest index; n = column i0 of V, not
                re-normalised; tr = (lam_0 + lam_1) + lam_2; curvature = max(lam_i0, 0) / tr rounded once to float32.  With
                tr <= 0 (all neighbours coincide) n = (0, 0, 0) and curvature = 0
  orientation   with a viewpoint v (three finite numbers, converted to float32): w = v - p_i in float64,
                s = (n_0*w_0 + n_1*w_1) + n_2*w_2, n is negated when s < 0.  Without a viewpoint, or when s == 0: n is
                negated when the first non-zero of (n_2, n_1, n_0) is negative - "upward", for terrestrial scans.  Then n
                is rounded to float32
  refusals      all ValueError, made on the host before any upload: bad shapes, non-finite coordinates, k outside 3 .. 64,
                M < k, M >= 2^31 - 1, a viewpoint that is not three finite numbers
"""
from collections import namedtuple

import numpy as np

_F32 = np.float32
MIN_K, MAX_K = 3, 64            # MAX_K = RL_KNN_MAX_K
MAX_POINTS = 2 ** 31 - 1
SWEEPS = 6
_PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))      # (p, q, r)
_QUERY_BLOCK = 1 << 16          # queries per call of the host K-NN: bounds the twin's memory at ~100 * k bytes each

NormalResult = namedtuple("NormalResult", ["normals", "curvature"])


def check_inputs(xyz, k, viewpoint):
    """The refusals of estimate_normals, all ValueError, made on the host (before any upload).  Returns the (M, 3) float32
    coordinates, k as int and the viewpoint as (3,) float32 (or None)."""
    if isinstance(k, bool) or int(k) != k or not MIN_K <= int(k) <= MAX_K:
        raise ValueError(f"estimate_normals: k={k!r} must be an integer in {MIN_K} .. {MAX_K}")
    k = int(k)
    shape = tuple(np.shape(xyz))
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"estimate_normals: xyz has shape {shape}, expected (M, 3)")
    M = shape[0]
    if M < k or M >= MAX_POINTS:             # (before anything is converted or copied)
        raise ValueError(f"estimate_normals: M={M} points, outside k={k} .. 2^31 - 2")
    with np.errstate(over="ignore"):            # (a coordinate beyond float32 becomes infinite and is refused below)
        pts = np.ascontiguousarray(np.asarray(xyz).astype(_F32))
    bad = ~np.isfinite(pts)
    if bad.any():
        i = int(np.flatnonzero(bad.any(axis=1))[0])
        raise ValueError(f"estimate_normals: non-finite coordinates, first at point {i}: {pts[i].tolist()}")
    if viewpoint is not None:
        try:
            with np.errstate(over="ignore"):
                v = np.asarray(viewpoint, dtype=np.float64).astype(_F32)
        except (TypeError, ValueError):
            raise ValueError(f"estimate_normals: viewpoint={viewpoint!r} must be three finite numbers") from None
        if v.shape != (3,) or not np.isfinite(v).all():
            raise ValueError(f"estimate_normals: viewpoint={viewpoint!r} must be three finite numbers")
        viewpoint = np.ascontiguousarray(v)
    return pts, k, viewpoint


def _neighbours(pts: np.ndarray, first: int, last: int, k: int) -> np.ndarray:
    """(last - first, k) int64: the library's host K-NN of the queries first .. last-1 in the whole cloud."""
    import torch
    from .. import _cpu
    t = torch.from_numpy(pts)
    idx, _ = _cpu.knn_host(t[None], t[None, first:last], k)
    return idx[0].numpy()


def _covariance(P: np.ndarray) -> np.ndarray:
    """P (Q, k, 3) float32 neighbour rows in rank order -> (Q, 6) float64 covariances (00, 01, 02, 11, 12, 22)."""
    Q, k, _ = P.shape
    P = P.astype(np.float64)
    mu = np.zeros((Q, 3), np.float64)
    for j in range(k):
        mu = mu + P[:, j]
    mu = mu / np.float64(k)
    C = np.zeros((Q, 6), np.float64)
    for j in range(k):
        d = P[:, j] - mu
        e = 0
        for a in range(3):
            for b in range(a, 3):
                C[:, e] = C[:, e] + d[:, a] * d[:, b]
                e += 1
    return C / np.float64(k)


def jacobi(C: np.ndarray):
    """The 6 cyclic Jacobi sweeps of the contract over (Q, 6) float64 covariances.  Returns (lam (Q, 3), V (Q, 3, 3)), the
    diagonal of A and the accumulated rotations (eigenvectors in columns)."""
    Q = C.shape[0]
    A = np.zeros((Q, 3, 3), np.float64)
    A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2] = (C[:, e] for e in range(6))
    V = np.zeros((Q, 3, 3), np.float64)
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1.0
    up = lambda i, j: (min(i, j), max(i, j))         # the upper triangle holds the symmetric matrix
    with np.errstate(all="ignore"):                  # (a skipped pair computes 0 / 0 and is not used)
        for _ in range(SWEEPS):
            for p, q, r in _PAIRS:
                apq, app, aqq = A[:, p, q], A[:, p, p], A[:, q, q]
                skip = apq == 0.0
                theta = (aqq - app) / (2.0 * apq)
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                arp, arq = A[(slice(None),) + up(r, p)], A[(slice(None),) + up(r, q)]
                new_pp, new_qq = app - t * apq, aqq + t * apq
                new_rp, new_rq = c * arp - s * arq, s * arp + c * arq
                A[:, p, p] = np.where(skip, app, new_pp)
                A[:, q, q] = np.where(skip, aqq, new_qq)
                A[(slice(None),) + up(r, p)] = np.where(skip, arp, new_rp)
                A[(slice(None),) + up(r, q)] = np.where(skip, arq, new_rq)
                A[:, p, q] = 0.0                     # (zero already where the pair was skipped)
                for i in range(3):
                    vip, viq = V[:, i, p], V[:, i, q]
                    new_p, new_q = c * vip - s * viq, s * vip + c * viq
                    V[:, i, p] = np.where(skip, vip, new_p)
                    V[:, i, q] = np.where(skip, viq, new_q)
    return np.stack((A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]), axis=1), V


def smallest(lam: np.ndarray, V: np.ndarray):
    """(n (Q, 3) un-oriented, curvature (Q,)), both float64 - before their one rounding to float32 - from jacobi's output:
    the column of the smallest eigenvalue (ties to the lowest index) and its share of the trace; zeros where the trace is
    not positive."""
    Q = lam.shape[0]
    i0 = np.zeros(Q, np.int64)
    i0 = np.where(lam[:, 1] < lam[np.arange(Q), i0], 1, i0)
    i0 = np.where(lam[:, 2] < lam[np.arange(Q), i0], 2, i0)
    n = V[np.arange(Q), :, i0]
    tr = (lam[:, 0] + lam[:, 1]) + lam[:, 2]
    flat = ~(tr > 0.0)
    with np.errstate(all="ignore"):
        curv = np.maximum(lam[np.arange(Q), i0], 0.0) / tr
    n = np.where(flat[:, None], 0.0, n)
    return n, np.where(flat, 0.0, curv)


def orient(n: np.ndarray, pts: np.ndarray, viewpoint) -> np.ndarray:
    """n (Q, 3) float64 turned towards the viewpoint, or upward without one or where it cannot decide; see the contract."""
    up = np.where(n[:, 2] != 0.0, n[:, 2] < 0.0, np.where(n[:, 1] != 0.0, n[:, 1] < 0.0, n[:, 0] < 0.0))
    if viewpoint is None:
        neg = up
    else:
        w = viewpoint.astype(np.float64)[None, :] - pts.astype(np.float64)
        s = (n[:, 0] * w[:, 0] + n[:, 1] * w[:, 1]) + n[:, 2] * w[:, 2]
        neg = np.where(s == 0.0, up, s < 0.0)
    return np.where(neg[:, None], -n, n)


def _blocks(M: int):
    for first in range(0, M, _QUERY_BLOCK):
        yield first, min(M, first + _QUERY_BLOCK)


def covariances_host(xyz, k: int = 16) -> np.ndarray:
    """(M, 6) float64: the neighbourhood covariances of the contract, entries (00, 01, 02, 11, 12, 22) - what the tests
    compare the kernel's cov_out and numpy's eigh with."""
    pts, k, _ = check_inputs(xyz, k, None)
    out = np.empty((pts.shape[0], 6), np.float64)
    for first, last in _blocks(pts.shape[0]):
        out[first:last] = _covariance(pts[_neighbours(pts, first, last, k)])
    return out


def estimate_normals_host(xyz, k: int = 16, viewpoint=None) -> NormalResult:
    """The numpy twin of the device estimation; see the module docstring for the contract.  Returns NormalResult(normals
    (M, 3) float32, curvature (M,) float32).  The neighbours come from the library's host K-NN (rl_knn_f32_cpu) in blocks
    of queries; a missing library raises."""
    pts, k, viewpoint = check_inputs(xyz, k, viewpoint)
    M = pts.shape[0]
    normals, curvature = np.empty((M, 3), _F32), np.empty(M, _F32)
    for first, last in _blocks(M):
        lam, V = jacobi(_covariance(pts[_neighbours(pts, first, last, k)]))
        n, curv = smallest(lam, V)
        curvature[first:last] = curv.astype(_F32)
        normals[first:last] = orient(n, pts[first:last], viewpoint).astype(_F32)
    return NormalResult(normals, curvature)


def estimate_normals(xyz, k: int = 16, viewpoint=None, device=None) -> NormalResult:
    """Normals (M, 3) and curvature (M,) of a cloud (M, 3) from every point's k nearest neighbours, turned towards
    `viewpoint` (the sensor's position) or upward without one.  Runs on the GPU (rl_knn_f32 + csrc/normals.hip) when
    `device` is a cuda device, or when it is None and one is available; otherwise estimate_normals_host.  Either way the
    result is numpy arrays, and the same ones bit for bit."""
    import torch
    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device(device)
    if device.type != "cuda":
        return estimate_normals_host(xyz, k, viewpoint)
    from .. import _ops as ops
    pts, k, viewpoint = check_inputs(xyz, k, viewpoint)
    with torch.cuda.device(device), torch.no_grad():
        n, c = ops.estimate_normals(torch.from_numpy(pts).to(device), k, viewpoint)
        return NormalResult(n.cpu().numpy(), c.cpu().numpy())


def normal_features(xyz, k: int = 16, viewpoint=None, device=None) -> np.ndarray:
    """(M, 4) float32 feature columns [n_x, n_y, n_z, curvature] of estimate_normals."""
    res = estimate_normals(xyz, k, viewpoint, device)
    return np.ascontiguousarray(np.concatenate((res.normals, res.curvature[:, None]), axis=1))


def rotate_columns(features: np.ndarray, column: int, R: np.ndarray) -> np.ndarray:
    """features (n, F) with the direction in columns column .. column+2 turned by R (3, 3) as the augmentation turns the
    centred coordinates: n'_r = (n_x*R[r,0] + n_y*R[r,1]) + n_z*R[r,2] in float64, rounded to the features' type.  A copy."""
    out = np.array(features, copy=True)
    n = np.asarray(features[:, column:column + 3], dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    for r in range(3):
        out[:, column + r] = (n[:, 0] * R[r, 0] + n[:, 1] * R[r, 1]) + n[:, 2] * R[r, 2]
    return out
