"""Fast point feature histograms (FPFH) of a point cloud and their nearest-neighbour matching: what a global, feature-based
registration pairs the points of two scans by when no initial pose is known (PCL's FPFHEstimation, Open3D's
compute_fpfh_feature).  A descriptor of 33 numbers per point - three histograms of 11 bins over the angles between the
point's normal and those of its neighbours - that does not change when the cloud is moved rigidly.

This module is the numpy host twin of csrc/fpfh.hip and csrc/match.hip (include/rl_randlanet.h, rl_fpfh_*, rl_match_u8) and
the public fpfh / fpfh_host / match_features / match_features_host.  The twin's arithmetic is the specification; the kernels
equal it bit for bit.  Everything below is float32, one correctly rounded operation at a time, nothing fused; division and
square root are true (correctly rounded) operations; no libm function is called anywhere:

  coordinates    converted to float32 first; every coordinate finite; k + 1 <= M < 2^31 - 1
  k              an integer, 2 <= k <= 63: the search is for k + 1 rows and RL_KNN_MAX_K is 64
  normals        the caller's (M, 3), converted to float32, every entry finite, or estimate_normals(xyz, k=normal_k,
                 viewpoint=viewpoint) of utils/normals.py on the same device (3 <= normal_k <= 64, normal_k <= M)
  neighbours     of point i: the ranks 1 .. k of the k + 1 rows of the project's exact K-NN with support = query = the cloud
                 (rl_knn_f32 / rl_knn_f32_cpu): d2 in un-fused float32, ascending by (d2, index).  Rank 0 is the point itself
                 or a coincident copy; a copy among the ranks 1 .. k has d2 = 0 and is skipped below
  pair (i, j)    Rusu's Darboux frame, the source always i: d = p_j - p_i per component; dist = sqrt(d2) with d2 the K-NN's
                 own value; dn = d / dist; u = n_i; v = dn x u = (dny*uz - dnz*uy, dnz*ux - dnx*uz, dnx*uy - dny*ux), each
                 product rounded, then the difference; lv2 = (vx*vx + vy*vy) + vz*vz; v = v / sqrt(lv2);
                 w = u x v by the same rule; with dot(a, b) = (ax*bx + ay*by) + az*bz:
                 f1 = dot(v, n_j), f2 = dot(u, dn), x = dot(u, n_j), y = dot(w, n_j).
                 The pair is SKIPPED, and counts nowhere, when d2 = 0, when lv2 is 0 or not finite (a neighbour straight
                 along the normal, an overflow), or when n_i or n_j is all zero
  bins           11 per feature.  bin(t) = 10 when t >= 10, trunc(t) when 0 < t < 10, 0 otherwise (a NaN gives 0).
                 b1 = bin((f1 + 1) * 5.5), b2 = bin((f2 + 1) * 5.5).  b3 = bin(a * 2.75) with a in [0, 4] the DIAMOND
                 PSEUDO-ANGLE of (x, y), measured from the negative x axis as atan2's range (-pi, pi] is: s = |x| + |y|;
                 a = 0 unless s > 0; r = y / s; a = 2 + r when x > 0, a = 4 - r when x <= 0 and y >= 0, a = 0 - r otherwise.
                 a is monotone in atan2(y, x) - equal normals give a = 2, the middle of the range, as they give PCL's
                 angle 0 - and needs additions and one division only; its bins are NOT uniform in the angle.  That is the
                 one deliberate difference from PCL, whose third feature is atan2(y, x) itself: the histogram is as
                 invariant and as descriptive, but not PCL's numbers
  SPFH           spfh[i][b1] += 1, spfh[i][11 + b2] += 1, spfh[i][22 + b3] += 1 per counted pair: integers <= 63, uint8
  FPFH           per bin b, from acc = 0 in rank order r = 1 .. k, with j_r the neighbour and w_r = 1 / d2_r:
                 acc = acc + float32(spfh[j_r][b]) * w_r.  A rank with d2_r = 0 or a w_r that is not finite is skipped.
                 There is no self term (PCL's rule).  Each of the three sub-histograms is then scaled: S = the sum of its
                 11 values from 0 in bin order; F[b] = acc[b] * (100 / S) when 0 < S < infinity, otherwise 0
  code           c[b] = 255 when t >= 255, trunc(t) when t > 0, else 0, with t = F[b] * 2.55 + 0.5 (float32 constants); 36
                 bytes per point, the last three 0: nine 4-byte words for the packed dot product of the matching
  outputs        FpfhResult(descriptor (M, 33) float32, code (M, 36) uint8, spfh (M, 33) uint8, normals (M, 3) float32)
  matching       match_features(code_source (Ms, 36), code_target (Mt, 36)) -> (idx (Ms,) int64, dist (Ms,) int32): for every
                 source row the target row of the smallest sum over the 36 bytes of (cs - ct)^2 - an exact integer, at most
                 33 * 255^2, so no summation order matters -, ties to the lowest target index.  1 <= Ms, Mt < 2^31 - 1
  refusals       all ValueError, made on the host before any upload, naming the argument

Not here: radius neighbourhoods (PCL's setRadiusSearch); other descriptors (SHOT, 3DSC); mutual (two-way) matching and
ratio tests - utils/registration.py's global_registration takes every source point's best match.
"""
from collections import namedtuple

import numpy as np

from . import normals as N

_F32 = np.float32
MIN_K, MAX_K = 2, N.MAX_K - 1       # the search is for k + 1 rows, at most RL_KNN_MAX_K
MAX_POINTS = 2 ** 31 - 1
BINS = 11
DIM = 3 * BINS                      # 33
CODE = 36                           # bytes of a code row: DIM rounded up to whole 4-byte words
_MATCH_BLOCK = 1 << 22              # source-target pairs the matching twin holds at a time

FpfhResult = namedtuple("FpfhResult", ["descriptor", "code", "spfh", "normals"])


def _integer(value, lo, hi, what):
    try:
        ok = not isinstance(value, (bool, str, bytes)) and int(value) == value and lo <= int(value) <= hi
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"{what}={value!r} must be an integer in {lo} .. {hi}")
    return int(value)


def check_inputs(xyz, k, normals, normal_k, viewpoint, who="fpfh", name="xyz"):
    """The refusals of fpfh, all ValueError, made on the host (before any upload).  Returns (pts (M, 3) float32, k, normals
    (M, 3) float32 or None, normal_k, viewpoint (3,) float32 or None)."""
    k = _integer(k, MIN_K, MAX_K, f"{who}: k")
    shape = tuple(np.shape(xyz))
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"{who}: {name} has shape {shape}, expected (M, 3)")
    M = shape[0]
    if M < k + 1 or M >= MAX_POINTS:            # (before anything is converted or copied)
        raise ValueError(f"{who}: {name} has M={M} points, outside k + 1 = {k + 1} .. 2^31 - 2")
    with np.errstate(over="ignore"):            # (a coordinate beyond float32 becomes infinite and is refused below)
        pts = np.ascontiguousarray(np.asarray(xyz).astype(_F32))
    bad = ~np.isfinite(pts)
    if bad.any():
        i = int(np.flatnonzero(bad.any(axis=1))[0])
        raise ValueError(f"{who}: {name} has non-finite coordinates, first at point {i}: {pts[i].tolist()}")
    if normals is not None:
        if tuple(np.shape(normals)) != (M, 3):
            raise ValueError(f"{who}: normals of {name} have shape {tuple(np.shape(normals))}, expected ({M}, 3)")
        with np.errstate(over="ignore"):
            nrm = np.ascontiguousarray(np.asarray(normals).astype(_F32))
        if not np.isfinite(nrm).all():
            raise ValueError(f"{who}: normals of {name} have non-finite entries")
        return pts, k, nrm, None, None
    nk = _integer(normal_k, N.MIN_K, N.MAX_K, f"{who}: normal_k")
    if M < nk:
        raise ValueError(f"{who}: {name} has M={M} points, fewer than normal_k={nk}: give normals")
    if viewpoint is not None:
        try:
            with np.errstate(over="ignore"):
                v = np.asarray(viewpoint, dtype=np.float64).astype(_F32)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: viewpoint={viewpoint!r} must be three finite numbers") from None
        if v.shape != (3,) or not np.isfinite(v).all():
            raise ValueError(f"{who}: viewpoint={viewpoint!r} must be three finite numbers")
        viewpoint = np.ascontiguousarray(v)
    return pts, k, None, nk, viewpoint


def check_codes(code, name, who="match_features"):
    """A code array: (M, 36) uint8 with 1 <= M < 2^31 - 1, contiguous."""
    c = np.asarray(code)
    if c.ndim != 2 or c.shape[1] != CODE or c.dtype != np.uint8 or not 1 <= c.shape[0] < MAX_POINTS:
        raise ValueError(f"{who}: {name} has shape {tuple(c.shape)} and dtype {c.dtype}, expected (M, {CODE}) uint8 with "
                         f"1 <= M < 2^31 - 1")
    return np.ascontiguousarray(c)


# ------------------------------------------------------------------------------------------------------------ the twin
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _bin(t, top):
    """bin(t) of the contract with the last bin `top`: top when t >= top, trunc(t) when 0 < t < top, else 0 (NaN: 0)."""
    return np.where(t > 0, np.minimum(t, _F32(top)), _F32(0)).astype(np.int32)


def pseudo_angle(x, y):
    """The diamond pseudo-angle a in [0, 4] of the contract, float32."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = np.abs(x) + np.abs(y)
        r = y / s
        a = np.where(x > 0, _F32(2) + r, np.where(y >= 0, _F32(4) - r, _F32(0) - r))
        return np.where(s > 0, a, _F32(0)).astype(_F32)


def pair_features_host(pts, nrm, i, j, d2):
    """The pair rule of the contract for the index arrays i, j (any one shape) and the K-NN's d2 of that shape: (f1, f2, x, y
    float32, counted bool)."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        pi, pj = pts[i], pts[j]
        ni, nj = nrm[i], nrm[j]
        dist = np.sqrt(d2)
        dn = tuple((pj[..., a] - pi[..., a]) / dist for a in range(3))
        u = tuple(ni[..., a] for a in range(3))
        n2 = tuple(nj[..., a] for a in range(3))
        v = _cross(dn, u)
        lv2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        lv = np.sqrt(lv2)
        v = tuple(c / lv for c in v)
        w = _cross(u, v)
        f1, f2, x, y = _dot(v, n2), _dot(u, dn), _dot(u, n2), _dot(w, n2)
        counted = (d2 != 0) & (lv2 > 0) & np.isfinite(lv2) & (ni != 0).any(axis=-1) & (nj != 0).any(axis=-1)
    assert f1.dtype == _F32 and y.dtype == _F32
    return f1, f2, x, y, counted


def bins_host(f1, f2, x, y):
    """(b1, b2, b3) int32 of the contract."""
    with np.errstate(invalid="ignore", over="ignore"):
        b1 = _bin((f1 + _F32(1)) * _F32(5.5), BINS - 1)
        b2 = _bin((f2 + _F32(1)) * _F32(5.5), BINS - 1)
        b3 = _bin(pseudo_angle(x, y) * _F32(2.75), BINS - 1)
    return b1, b2, b3


def spfh_host(pts, nrm, idx, d2):
    """(M, 33) uint8: idx, d2 (M, k + 1) the K-NN rows."""
    M = pts.shape[0]
    hist = np.zeros((M, DIM), np.int32)
    i = np.broadcast_to(np.arange(M)[:, None], (M, idx.shape[1] - 1))
    f1, f2, x, y, counted = pair_features_host(pts, nrm, i, idx[:, 1:], d2[:, 1:])
    b1, b2, b3 = bins_host(f1, f2, x, y)
    rows = i[counted]
    for off, b in ((0, b1), (BINS, b2), (2 * BINS, b3)):
        np.add.at(hist, (rows, off + b[counted]), 1)
    return hist.astype(np.uint8)


def fpfh_from_spfh_host(spfh, idx, d2):
    """(descriptor (M, 33) float32, code (M, 36) uint8) of the contract."""
    M, k1 = idx.shape
    acc = np.zeros((M, DIM), _F32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for r in range(1, k1):
            w = _F32(1) / d2[:, r]
            use = (d2[:, r] != 0) & np.isfinite(w)
            term = spfh[idx[:, r]].astype(_F32) * w[:, None]
            acc = np.where(use[:, None], acc + term, acc)
        out = np.zeros((M, DIM), _F32)
        for h in range(3):
            part = acc[:, h * BINS:(h + 1) * BINS]
            S = np.zeros(M, _F32)
            for b in range(BINS):
                S = S + part[:, b]
            ok = (S > 0) & np.isfinite(S)
            scale = _F32(100) / S
            out[:, h * BINS:(h + 1) * BINS] = np.where(ok[:, None], part * scale[:, None], _F32(0))
        t = out * _F32(2.55) + _F32(0.5)
    assert out.dtype == _F32 and t.dtype == _F32
    code = np.zeros((M, CODE), np.uint8)
    code[:, :DIM] = np.where(t > 0, np.minimum(t, _F32(255)), _F32(0)).astype(np.uint8)
    return out, code


def _knn_rows(pts, k1):
    """(idx (M, k1) int64, d2 (M, k1) float32): the library's host K-NN of the cloud in itself, in blocks of queries."""
    import torch
    from .. import _cpu
    M = pts.shape[0]
    idx, d2 = np.empty((M, k1), np.int64), np.empty((M, k1), _F32)
    t = torch.from_numpy(pts)
    for first, last in N._blocks(M):
        i, d = _cpu.knn_host(t[None], t[None, first:last], k1)
        idx[first:last], d2[first:last] = i[0].numpy(), d[0].numpy()
    return idx, d2


def _fpfh_checked_host(pts, k, nrm, nk, viewpoint) -> FpfhResult:
    if nrm is None:
        nrm = N.estimate_normals_host(pts, nk, viewpoint).normals
    idx, d2 = _knn_rows(pts, k + 1)
    spfh = spfh_host(pts, nrm, idx, d2)
    desc, code = fpfh_from_spfh_host(spfh, idx, d2)
    return FpfhResult(desc, code, spfh, nrm)


def _host_array(x):
    import torch
    return x.detach().cpu().numpy() if torch.is_tensor(x) else x


def fpfh_host(xyz, k=30, normals=None, normal_k=16, viewpoint=None) -> FpfhResult:
    """The numpy twin of the device descriptor; see the module docstring for the contract.  The neighbours come from the
    library's host K-NN (rl_knn_f32_cpu); a missing library raises."""
    return _fpfh_checked_host(*check_inputs(_host_array(xyz), k, None if normals is None else _host_array(normals),
                                            normal_k, viewpoint))


def match_features_host(code_source, code_target):
    """The numpy twin of rl_match_u8: (idx (Ms,) int64, dist (Ms,) int32)."""
    cs, ct = check_codes(code_source, "code_source"), check_codes(code_target, "code_target")
    return _match_checked_host(cs, ct)


def _match_checked_host(cs, ct):
    Ms, Mt = cs.shape[0], ct.shape[0]
    a, b = cs.astype(_F32), ct.astype(_F32)         # (float32 is exact here: every partial sum is an integer below 2^24)
    na, nb = (a * a).sum(axis=1).astype(np.int32), (b * b).sum(axis=1).astype(np.int32)
    idx, dist = np.zeros(Ms, np.int64), np.full(Ms, np.iinfo(np.int32).max, np.int32)
    sstep = max(1, min(Ms, 4096))
    tstep = max(1, _MATCH_BLOCK // sstep)
    for s in range(0, Ms, sstep):
        for t in range(0, Mt, tstep):           # ascending target blocks and a strict <: ties to the lowest index
            d = na[s:s + sstep, None] + nb[None, t:t + tstep] - 2 * (a[s:s + sstep] @ b[t:t + tstep].T).astype(np.int32)
            j = d.argmin(axis=1)                # the first minimum
            dj = d[np.arange(d.shape[0]), j].astype(np.int32)
            better = dj < dist[s:s + sstep]
            idx[s:s + sstep] = np.where(better, j + t, idx[s:s + sstep])
            dist[s:s + sstep] = np.where(better, dj, dist[s:s + sstep])
    return idx, dist


# --------------------------------------------------------------------------------------------------------- device path
def _cuda(device, *arrays):
    import torch
    if device is None:
        for c in arrays:
            if torch.is_tensor(c) and c.is_cuda:
                device = c.device
                break
        else:
            device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device(device)
    return device if device.type == "cuda" else None


def fpfh_device(pts, k, nrm, nk, viewpoint, device):
    """fpfh of checked arguments (check_inputs; pts and nrm numpy arrays or float32 tensors on `device`) on a cuda device:
    (descriptor, code, spfh, normals) as device tensors."""
    import torch
    from .. import _ops as ops
    with torch.cuda.device(device), torch.no_grad():
        p = (pts if torch.is_tensor(pts) else torch.from_numpy(pts)).to(device)
        if nrm is None:
            n = ops.estimate_normals(p, nk, viewpoint)[0]
        else:
            n = (nrm if torch.is_tensor(nrm) else torch.from_numpy(nrm)).to(device)
        desc, code, spfh = ops.fpfh(p, n, k)
        return desc, code, spfh, n


def fpfh(xyz, k=30, normals=None, normal_k=16, viewpoint=None, device=None) -> FpfhResult:
    """The FPFH descriptor of every point of a cloud (M, 3): FpfhResult(descriptor, code, spfh, normals) - see the module
    docstring.  Runs on the GPU (rl_knn_f32, rl_normals, csrc/fpfh.hip) when `device` is a cuda device, or when it is None
    and one is available; otherwise fpfh_host.  Either way the result is numpy arrays, and the same ones bit for bit."""
    dev = _cuda(device)
    args = check_inputs(_host_array(xyz), k, None if normals is None else _host_array(normals), normal_k, viewpoint)
    if dev is None:
        return _fpfh_checked_host(*args)
    return FpfhResult(*(t.cpu().numpy() for t in fpfh_device(*args, dev)))


def match_features(code_source, code_target, device=None):
    """For every row of code_source (Ms, 36) uint8 the nearest row of code_target (Mt, 36) uint8: (idx (Ms,) int64, dist
    (Ms,) int32) - see the module docstring.  On the GPU (csrc/match.hip) when `device` is a cuda device, or when it is None
    and one is available; otherwise match_features_host.  The same arrays bit for bit either way."""
    dev = _cuda(device)
    cs, ct = check_codes(_host_array(code_source), "code_source"), check_codes(_host_array(code_target), "code_target")
    if dev is None:
        return _match_checked_host(cs, ct)
    import torch
    from .. import _ops as ops
    with torch.cuda.device(dev), torch.no_grad():
        idx, dist = ops.match_features(torch.from_numpy(cs).to(dev), torch.from_numpy(ct).to(dev))
        return idx.cpu().numpy(), dist.cpu().numpy()
