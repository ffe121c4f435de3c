"""Rigid registration of two overlapping point clouds by iterative closest point (ICP): a second depth camera on the other
side of the desk, a handheld camera moving through a room, the stations of a terrestrial scan are brought into one frame
before anything else looks at them (PCL's IterativeClosestPoint, Open3D's registration_icp).  The source is moved until
every one of its points lies on the target's surface (point to plane) or on its nearest target point (point to point).

This module is the numpy host twin of csrc/icp.hip (include/rl_randlanet.h, rl_icp_*) and the public icp / icp_host /
apply_transform / evaluate_registration.  The twin's arithmetic is the specification; the kernels equal it bit for bit:

  clouds         source (Ms, 3) and target (Mt, 3), converted to float32 first; every coordinate finite;
                 1 <= Ms < 2^31 - 1 and 1 <= Mt < 2^31 - 1
  max_distance   finite and > 0, rounded once to float32: md32; the gate is g2 = md32 * md32, rounded once to float32
  iterations     an integer in 0 .. 256: the maximum number of updates
  init           a (4, 4) float64 rigid transform, the identity by default
  normals        metric="point_to_plane" needs the target's: target_normals (Mt, 3) float32 if given, otherwise
                 estimate_normals(target, k=normals) of utils/normals.py on the same device as the rest, which needs
                 Mt >= normals.  The sign of a normal does not matter - every term below is even in n -, and a zero normal
                 contributes zeros and still counts as a pair
  state          T, a (4, 4) float64 array.  One EVALUATION of T is the next five steps
  transform      R32 = float32(T[:3, :3]), t32 = float32(T[:3, 3]); q_i = ((R00*x + R01*y) + R02*z) + tx, and likewise for
                 the rows 1 and 2: float32, one rounded operation at a time, nothing fused
  correspondence (j_i, d2_i) = the exact 1-NN of q_i in the target by the library's K-NN contract (rl_knn_f32 /
                 rl_knn_f32_cpu): d2 in un-fused float32, ties to the lowest index.  Pair i is VALID iff d2_i <= g2
  terms          of a valid pair, in float64, every product rounded before it is added: p = q_i, y = target[j_i],
                 n = normal[j_i], d = p - y; r = (d0*n0 + d1*n1) + d2*n2;
                 a = (p1*n2 - p2*n1, p2*n0 - p0*n2, p0*n1 - p1*n0); J = (a0, a1, a2, n0, n1, n2).  The 29 columns: the 21
                 products J_u*J_v, u <= v, row-major upper triangle; the 6 products J_u*r; r*r; float64(d2_i).  An invalid
                 pair contributes +0.0 in every column, so the order of every sum is a function of Ms alone.
                 metric="point_to_point": the same rule three times, with n = e_0, e_1, e_2, the three results added per
                 column in that order, (c^0 + c^1) + c^2; the d2 column is taken once
  sums           every column by boxes.fixed_sums with one id whose members are the source points 0 .. Ms-1: chunks of 1024,
                 64 lanes x 16 turns, the fold in halves, then the chunk sums through the same two steps.  count = the
                 number of valid pairs, an exact integer
  scores         fitness = count / Ms; inlier_rmse = sqrt(D / count) with D the sum of the d2 column, 0 when count is 0
  stop           BEFORE updating, when (a) this is not the first evaluation and |fitness - previous| < relative_fitness and
                 |inlier_rmse - previous| < relative_rmse: status "converged"; (b) `iterations` updates are done: status
                 "iterations"; (c) count < min_pairs, or np.linalg.solve raises, or the step is not finite: "degenerate"
  update         host float64, the same code on both paths: A the symmetric 6x6 matrix of the 21 sums, b the 6 sums,
                 x = solve(A, -b); w = x[:3], theta = |w|; dR = I when theta == 0, otherwise I + sin(theta) K +
                 (1 - cos(theta)) K K with K the cross matrix of w / theta; dt = x[3:]; T <- dT @ T
  outputs        RegistrationResult(transformation (4, 4) float64, fitness, inlier_rmse, count, updates, status,
                 correspondence (Ms,) int64 - j_i, -1 for an invalid pair -, history (evaluations, 30) float64 - count and
                 the 29 sums of every evaluation -, transformed (Ms, 3) float32 - q).  All fields belong to the returned T:
                 they are those of the last evaluation
  refusals       all ValueError, made on the host before any upload, naming the argument

GLOBAL REGISTRATION - an initial pose for ICP when the caller has none: the second camera 90 to 180 degrees round the desk,
a lost frame, two scanner stations without extrinsics (PCL's SampleConsensusPrerejective, Open3D's
registration_ransac_based_on_feature_matching).  global_registration / global_registration_host, the twin of csrc/global.hip
(rl_global_*); float32, one correctly rounded operation at a time, nothing fused, true division and square root, no libm:

  clouds         as above, with 3 <= Ms and both clouds large enough for utils/features.py's fpfh (k + 1 and `normals` points)
  max_distance   as above: the gate is g2 = md32 * md32
  correspondence C = Ms of them: c = (c, j_c) with j_c = match_features(fpfh(source).code, fpfh(target).code) - the descriptors
                 with k, normal_k = `normals`, the cloud's viewpoint or the caller's normals (utils/features.py)
  triples        (T, 3) integers in [0, C): the caller's, or np.random.default_rng(seed).integers(0, C, (T, 3)) - a generator
                 of its own, drawn on the host for both paths; T = iterations in 1 .. 2^20
  hypothesis t   from a_m = source[tri_m], b_m = target[j_(tri_m)], m = 0, 1, 2.  The squared lengths of the edges a1 - a0,
                 a2 - a0, a2 - a1 and of the same on the b side, l = (ex*ex + ey*ey) + ez*ez.  It is VALID iff for each edge
                 la > 0, lb > 0, la >= s2 * lb and lb >= s2 * la, with s2 = es32 * es32 and es32 = float32(edge_similarity)
                 (PCL's polygonal pre-rejection), and every entry below is finite.  A frame per side from e1 = p1 - p0 and
                 e2 = p2 - p0: u = e1 / sqrt(l_e1); c = e1 x e2 (each product rounded, then the difference);
                 w = c / sqrt((cx*cx + cy*cy) + cz*cz); v = w x u.  R[r][s] = (ub[r]*ua[s] + vb[r]*va[s]) + wb[r]*wa[s];
                 t[r] = b0[r] - ((R[r][0]*a0x + R[r][1]*a0y) + R[r][2]*a0z).  Stored as twelve floats, R row-major then t;
                 an invalid hypothesis is twelve NaNs and counts 0.  Repeated indices and collinear triples are invalid by
                 these rules (a zero edge, a zero cross product: 0 / 0)
  score          q_c = R a_c + t by the transform rule above; e = q_c - b_c; e2 = (ex*ex + ey*ey) + ez*ez; correspondence c
                 is an INLIER iff e2 <= g2 (a NaN compares false).  counts[t] = the number of inliers, an exact integer
  best           the FIRST maximum of counts.  A maximum of 0: status "not_found", the identity, no inlier, best -1
  sums           under the best hypothesis, sixteen float64 columns summed by boxes.fixed_sums over c = 0 .. C-1 with +0.0
                 for a non-inlier: 1, a (3), b (3), a_u * b_v (9, u-major), every entry float64(float32 value)
  refinement     when the best count is >= 3: Kabsch on the host in float64, the same code on both paths: n = sums[0],
                 H = Sab - Sa Sb^T / n, U S V^T = svd(H), R = V diag(1, 1, det(V U^T)) U^T, t = Sb / n - R Sa / n: status
                 "refined".  The final `count` and `inlier` are the score rule once more with float32 of the refined
                 transform.  With a best count of 1 or 2, or an SVD that fails or is not finite, the hypothesis is kept
                 (as float64 of its float32 entries): status "hypothesis"
  outputs        GlobalRegistrationResult(transformation (4, 4) float64, count, fitness = count / C, inlier (C,) bool,
                 correspondence (Ms,) int64 = j_c, best, counts (T,) int32, hypotheses (T, 12) float32, sums (16,) float64 -
                 zeros when not found -, status)

Not here: scale estimation; robust kernels; colored or generalised ICP; clouds far from the origin: a = p x n is formed in
the caller's coordinates, so shift such scans first; a K-NN that keeps its grid between iterations: every evaluation builds
the target's grid again.  Of the global registration: mutual (two-way) filtering of the correspondences; radius
neighbourhoods; verifying several top hypotheses by the true 1-NN fitness instead of the correspondences' own; scale;
symmetric scenes, which no descriptor resolves.
"""
from collections import namedtuple
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import boxes as B
from . import normals as N

_F32 = np.float32
MAX_POINTS = 2 ** 31 - 1
MAX_ITERATIONS = 256
METRICS = ("point_to_plane", "point_to_point")      # the `metric` of rl_icp_sums is the index
COLUMNS = 29

RegistrationResult = namedtuple("RegistrationResult", ["transformation", "fitness", "inlier_rmse", "count", "updates", "status",
                                                       "correspondence", "history", "transformed"])
_Checked = namedtuple("_Checked", ["g2", "metric", "normals", "iterations", "init", "relative_fitness", "relative_rmse",
                                   "min_pairs"])


@dataclass(frozen=True)
class IcpSettings:
    """What Model.predict_views(icp=...) takes: the keywords of icp."""
    max_distance: float
    metric: str = "point_to_plane"
    normals: int = 16
    iterations: int = 30
    relative_fitness: float = 1e-6
    relative_rmse: float = 1e-6
    min_pairs: int = 6


def _integer(value, lo, hi, what):
    try:
        ok = not isinstance(value, (bool, str, bytes)) and int(value) == value and lo <= int(value) <= hi
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"{what}={value!r} must be an integer in {lo} .. {hi}")
    return int(value)


def _tolerance(value, what):
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{what}={value!r} must be a finite number >= 0") from None
    if isinstance(value, bool) or not np.isfinite(v) or v < 0.0:
        raise ValueError(f"{what}={value!r} must be a finite number >= 0")
    return v


def check_transform(T, what="icp: init"):
    """A (4, 4) float64 rigid transform: finite, last row (0, 0, 0, 1), R orthonormal within 1e-6 and det R > 0."""
    try:
        M = np.array(T, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a (4, 4) rigid transform") from None
    if M.shape != (4, 4) or not np.isfinite(M).all():
        raise ValueError(f"{what} must be a finite (4, 4) rigid transform, got shape {tuple(M.shape)}")
    R = M[:3, :3]
    if (M[3] != (0.0, 0.0, 0.0, 1.0)).any() or np.abs(R @ R.T - np.eye(3)).max() > 1e-6 or np.linalg.det(R) <= 0.0:
        raise ValueError(f"{what} is not a rigid transform: its rotation is not orthonormal or its last row is not (0, 0, 0, 1)")
    return M


def check_parameters(max_distance, metric="point_to_plane", normals=16, iterations=30, init=None, relative_fitness=1e-6,
                     relative_rmse=1e-6, min_pairs=6, who="icp") -> _Checked:
    """The refusals that do not depend on the clouds, all ValueError."""
    try:
        md = float(max_distance)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: max_distance={max_distance!r} must be a finite number > 0") from None
    with np.errstate(over="ignore"):
        md32 = _F32(md)
        g2 = md32 * md32
    if isinstance(max_distance, bool) or not np.isfinite(md32) or not md32 > 0 or not np.isfinite(g2) or not g2 > 0:
        raise ValueError(f"{who}: max_distance={max_distance!r} must be a finite number > 0 whose square is one in float32")
    if metric not in METRICS:
        raise ValueError(f"{who}: metric={metric!r} must be one of {METRICS}")
    k = _integer(normals, N.MIN_K, N.MAX_K, f"{who}: normals")
    it = _integer(iterations, 0, MAX_ITERATIONS, f"{who}: iterations")
    T = np.eye(4) if init is None else check_transform(init, f"{who}: init")
    rf = _tolerance(relative_fitness, f"{who}: relative_fitness")
    rr = _tolerance(relative_rmse, f"{who}: relative_rmse")
    mp = _integer(min_pairs, 1, MAX_POINTS - 1, f"{who}: min_pairs")
    return _Checked(g2, METRICS.index(metric), k, it, T, rf, rr, mp)


def check_cloud(xyz, name, who="icp", rows=None):
    """The refusals of one cloud (or of the normals, with rows = Mt), all ValueError.  Returns (M, 3) float32."""
    shape = tuple(np.shape(xyz))
    want = "(M, 3)" if rows is None else f"({rows}, 3)"
    if len(shape) != 2 or shape[1] != 3 or (rows is not None and shape[0] != rows):
        raise ValueError(f"{who}: {name} has shape {shape}, expected {want}")
    M = shape[0]
    if M < 1 or M >= MAX_POINTS:                    # (before anything is converted or copied)
        raise ValueError(f"{who}: {name} has M={M} points, outside 1 .. 2^31 - 2")
    with np.errstate(over="ignore"):                # (a coordinate beyond float32 becomes infinite and is refused below)
        pts = np.ascontiguousarray(np.asarray(xyz).astype(_F32))
    bad = ~np.isfinite(pts)
    if bad.any():
        i = int(np.flatnonzero(bad.any(axis=1))[0])
        raise ValueError(f"{who}: {name} has non-finite coordinates, first at row {i}: {pts[i].tolist()}")
    return pts


def check_normals_size(Mt, chk: _Checked, target_normals, who="icp"):
    if chk.metric == 0 and target_normals is None and Mt < chk.normals:
        raise ValueError(f"{who}: target has Mt={Mt} points, fewer than normals={chk.normals}: give target_normals")


# ------------------------------------------------------------------------------------------------- one evaluation, host
def transform_host(pts: np.ndarray, T: np.ndarray) -> np.ndarray:
    """The float32 transform of the contract: pts (M, 3) float32 moved by T (4, 4) float64."""
    R = T[:3, :3].astype(_F32)
    t = T[:3, 3].astype(_F32)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    q = np.empty_like(pts)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(3):
            q[:, a] = ((R[a, 0] * x + R[a, 1] * y) + R[a, 2] * z) + t[a]
    return q


def nearest_host(tgt: np.ndarray, q: np.ndarray):
    """(idx (Q,) int64, d2 (Q,) float32): the library's host 1-NN of q in tgt, in blocks of queries."""
    import torch
    from .. import _cpu
    idx, d2 = np.empty(q.shape[0], np.int64), np.empty(q.shape[0], _F32)
    s = torch.from_numpy(tgt)[None]
    for first, last in N._blocks(q.shape[0]):
        i, d = _cpu.knn_host(s, torch.from_numpy(q[first:last])[None], 1)
        idx[first:last], d2[first:last] = i[0, :, 0].numpy(), d[0, :, 0].numpy()
    return idx, d2


def _pair_columns(p, d, n):
    """The 28 columns that depend on the normal: p, d, n (M, 3) float64 -> (M, 28)."""
    r = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    J = (p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2], p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0],
         n[:, 0], n[:, 1], n[:, 2])
    cols = [J[u] * J[v] for u in range(6) for v in range(u, 6)] + [J[u] * r for u in range(6)] + [r * r]
    return np.stack(cols, axis=1)


def terms_host(q, tgt, nrm, idx, d2, valid, metric):
    """(Ms, 29) float64: the columns of the contract, +0.0 in the rows of invalid pairs."""
    p = q.astype(np.float64)
    d = p - tgt[idx].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        if metric == 0:
            c = _pair_columns(p, d, nrm[idx].astype(np.float64))
        else:
            e = np.eye(3)
            c0, c1, c2 = (_pair_columns(p, d, np.broadcast_to(e[a], p.shape)) for a in range(3))
            c = (c0 + c1) + c2
    c = np.concatenate((c, d2.astype(np.float64)[:, None]), axis=1)
    return np.where(valid[:, None], c, 0.0)


def evaluate_host(src, tgt, nrm, T, g2, metric):
    """One evaluation of T on the host: (row (30,) float64 = count and the 29 sums, correspondence (Ms,) int64, q)."""
    q = transform_host(src, T)
    idx, d2 = nearest_host(tgt, q)
    valid = d2 <= g2
    cols = terms_host(q, tgt, nrm, idx, d2, valid, metric)
    with np.errstate(over="ignore", invalid="ignore"):
        sums = B.fixed_sums(cols, np.array([src.shape[0]]))[0]
    row = np.concatenate(([np.float64(valid.sum())], sums))
    return row, np.where(valid, idx, -1).astype(np.int64), q


# ------------------------------------------------------------------------------------------- the iteration, both paths
def scores(row, Ms):
    """(count, fitness, inlier_rmse) of one evaluation's row."""
    count = int(row[0])
    return count, count / Ms, float(np.sqrt(row[COLUMNS] / np.float64(count))) if count else 0.0


def normal_equations(row):
    """(A (6, 6), b (6,)) float64 from one evaluation's row."""
    A = np.zeros((6, 6), np.float64)
    iu = np.triu_indices(6)                         # row-major upper triangle
    A[iu] = row[1:22]
    A[(iu[1], iu[0])] = row[1:22]
    return A, row[22:28].copy()


def step(row):
    """The update dT (4, 4) float64 of the contract from one evaluation's row, or None when there is none."""
    A, b = normal_equations(row)
    try:
        with np.errstate(all="ignore"):
            x = np.linalg.solve(A, -b)
    except np.linalg.LinAlgError:
        return None
    if not np.isfinite(x).all():
        return None
    w = x[:3]
    theta = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    dT = np.eye(4)
    if theta != 0.0:
        u = w / theta
        K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
        dT[:3, :3] = np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * (K @ K)
    dT[:3, 3] = x[3:]
    return dT if np.isfinite(dT).all() else None


def run(evaluate, Ms, chk: _Checked):
    """The iteration of the contract around evaluate(T) -> row (30,) float64: what the twin and the device path both call.
    Returns (T, fitness, inlier_rmse, count, updates, status, history)."""
    T = chk.init.copy()
    history, updates, previous = [], 0, None
    while True:
        row = np.asarray(evaluate(T), np.float64)
        history.append(row)
        count, fitness, rmse = scores(row, Ms)
        if previous is not None and abs(fitness - previous[0]) < chk.relative_fitness \
                and abs(rmse - previous[1]) < chk.relative_rmse:
            status = "converged"
            break
        if updates >= chk.iterations:
            status = "iterations"
            break
        dT = step(row) if count >= chk.min_pairs else None
        if dT is None:
            status = "degenerate"
            break
        T = dT @ T
        updates += 1
        previous = (fitness, rmse)
    return T, fitness, rmse, count, updates, status, np.array(history, np.float64).reshape(-1, COLUMNS + 1)


def _icp_checked_host(src, tgt, nrm, chk: _Checked) -> RegistrationResult:
    last = {}

    def evaluate(T):
        row, last["corr"], last["q"] = evaluate_host(src, tgt, nrm, T, chk.g2, chk.metric)
        return row

    T, fitness, rmse, count, updates, status, history = run(evaluate, src.shape[0], chk)
    return RegistrationResult(T, fitness, rmse, count, updates, status, last["corr"], history, last["q"])


def _host_array(x):
    import torch
    return x.detach().cpu().numpy() if torch.is_tensor(x) else x


def icp_host(source, target, *, max_distance, metric="point_to_plane", target_normals=None, normals=16, iterations=30,
             init=None, relative_fitness=1e-6, relative_rmse=1e-6, min_pairs=6) -> RegistrationResult:
    """The numpy twin of the device registration; see the module docstring for the contract.  The correspondences come from
    the library's host K-NN (rl_knn_f32_cpu); a missing library raises."""
    chk = check_parameters(max_distance, metric, normals, iterations, init, relative_fitness, relative_rmse, min_pairs)
    src = check_cloud(_host_array(source), "source")
    tgt = check_cloud(_host_array(target), "target")
    nrm = None
    if chk.metric == 0:
        check_normals_size(tgt.shape[0], chk, target_normals)
        nrm = (N.estimate_normals_host(tgt, chk.normals).normals if target_normals is None
               else check_cloud(_host_array(target_normals), "target_normals", rows=tgt.shape[0]))
    return _icp_checked_host(src, tgt, nrm, chk)


# ---------------------------------------------------------------------------------------------------------- device path
def _cuda(device, *clouds):
    """The cuda device to run on, or None for the host: `device`, else that of a cloud given as a device tensor, else cuda
    when there is one."""
    import torch
    if device is None:
        for c in clouds:
            if torch.is_tensor(c) and c.is_cuda:
                device = c.device
                break
        else:
            device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device(device)
    return device if device.type == "cuda" else None


def _checked_cloud(xyz, name, device, who="icp", rows=None):
    """A cloud for `device`, refused or not before anything is uploaded: a tensor that already lies on a cuda device is
    checked where it lies (one flag read back) and returned contiguous, anything else goes through check_cloud and is
    returned as a host tensor."""
    import torch
    if torch.is_tensor(xyz) and xyz.is_cuda:
        shape = tuple(xyz.shape)
        if (device.index is not None and xyz.device != device) or xyz.dtype != torch.float32 or len(shape) != 2 or shape[1] != 3 or not 1 <= shape[0] < MAX_POINTS \
                or (rows is not None and shape[0] != rows):
            raise ValueError(f"{who}: {name} is a {xyz.dtype} tensor of shape {shape} on {xyz.device}, expected float32 (M, 3) "
                             f"with 1 <= M < 2^31 - 1 on {device}")
        if not bool(torch.isfinite(xyz).all()):
            raise ValueError(f"{who}: {name} has non-finite coordinates")
        return xyz.contiguous()
    return torch.from_numpy(check_cloud(_host_array(xyz), name, who, rows))


def icp_device(source, target, target_normals, chk: _Checked, device, who="icp", chunk=1 << 20) -> RegistrationResult:
    """icp of checked parameters on a cuda device; `correspondence` and `transformed` of the result are device tensors, and
    so may `source`, `target` and `target_normals` be (Model.predict_views keeps the views there)."""
    import torch
    from .. import _ops as ops
    with torch.cuda.device(device), torch.no_grad():
        src = _checked_cloud(source, "source", device, who)
        tgt = _checked_cloud(target, "target", device, who)
        nrm = None
        if chk.metric == 0:
            check_normals_size(tgt.shape[0], chk, target_normals, who)
            if target_normals is not None:
                nrm = _checked_cloud(target_normals, "target_normals", device, who, rows=tgt.shape[0]).to(device)
        src, tgt = src.to(device), tgt.to(device)          # (every refusal was made above)
        if chk.metric == 0 and nrm is None:
            nrm = ops.estimate_normals(tgt, chk.normals)[0]
        return RegistrationResult(*ops.icp(src, tgt, nrm, chk, chunk=chunk))


def icp(source, target, *, max_distance, metric="point_to_plane", target_normals=None, normals=16, iterations=30, init=None,
        relative_fitness=1e-6, relative_rmse=1e-6, min_pairs=6, device=None) -> RegistrationResult:
    """The rigid transform that moves `source` (Ms, 3) onto `target` (Mt, 3): RegistrationResult(transformation, fitness,
    inlier_rmse, count, updates, status, correspondence, history, transformed) - see the module docstring.  Runs on the GPU
    (rl_icp_transform, rl_knn_f32, rl_icp_sums, rl_icp_fold per evaluation; the 6x6 solve on the host) when `device` is a cuda
    device, or when it is None and one is available; otherwise icp_host.  The clouds may be float32 tensors on that device -
    utils/depth.py's depth_points(..., device=...) makes such - and are then used where they lie.  Either way the result is
    numpy arrays, and the same ones bit for bit."""
    dev = _cuda(device, source, target)
    if dev is None:
        return icp_host(source, target, max_distance=max_distance, metric=metric, target_normals=target_normals, normals=normals,
                        iterations=iterations, init=init, relative_fitness=relative_fitness, relative_rmse=relative_rmse,
                        min_pairs=min_pairs)
    chk = check_parameters(max_distance, metric, normals, iterations, init, relative_fitness, relative_rmse, min_pairs)
    res = icp_device(source, target, target_normals, chk, dev)
    return res._replace(correspondence=res.correspondence.cpu().numpy(), transformed=res.transformed.cpu().numpy())


def evaluate_registration(source, target, T, max_distance, *, metric="point_to_plane", target_normals=None, normals=16,
                          device=None) -> RegistrationResult:
    """How well T (4, 4) registers source onto target: icp with init=T and iterations=0 - one evaluation, no update."""
    return icp(source, target, max_distance=max_distance, metric=metric, target_normals=target_normals, normals=normals,
               iterations=0, init=T, device=device)


def apply_transform(xyz, T, device=None):
    """xyz (M, 3) moved by the rigid transform T (4, 4) float64: the float32 transform of the contract, the same bits on both
    paths.  A numpy array gives a numpy array; a float32 tensor on a cuda device is moved there and gives a tensor."""
    import torch
    T = check_transform(T, "apply_transform: T")
    dev = _cuda(device, xyz)
    if dev is None:
        return transform_host(check_cloud(_host_array(xyz), "xyz", "apply_transform"), T)
    from .. import _ops as ops
    on_device = torch.is_tensor(xyz) and xyz.is_cuda
    with torch.cuda.device(dev), torch.no_grad():
        q = ops.icp_transform(_checked_cloud(xyz, "xyz", dev, "apply_transform").to(dev), T)
        return q if on_device else q.cpu().numpy()


# ------------------------------------------------------------------------------------------------- global registration
MAX_HYPOTHESES = 1 << 20            # RL_GLOBAL_MAX_HYPOTHESES
SUM_COLUMNS = 16                    # 1, a (3), b (3), a_u * b_v (9)
_SCORE_BLOCK = 1 << 22              # hypothesis-correspondence tests the twin holds at a time

GlobalRegistrationResult = namedtuple("GlobalRegistrationResult", ["transformation", "count", "fitness", "inlier", "correspondence",
                                                                   "best", "counts", "hypotheses", "sums", "status"])
_GlobalChecked = namedtuple("_GlobalChecked", ["g2", "k", "normals", "T", "seed", "s2"])


@dataclass(frozen=True)
class GlobalSettings:
    """What Model.predict_views(global_init=...) takes: the voxel both clouds are grid-subsampled with, then the keywords of
    global_registration.  max_distance None: 1.5 * voxel.  viewpoints None: every view's own origin (the depth camera);
    otherwise one (3,) position per view, in that view's frame."""
    voxel: float
    max_distance: Optional[float] = None
    k: int = 30
    normals: int = 16
    iterations: int = 65536
    seed: int = 0
    edge_similarity: float = 0.9
    viewpoints: Optional[Tuple] = None


def check_global_parameters(max_distance, k=30, normals=16, iterations=65536, seed=0, edge_similarity=0.9,
                            who="global_registration") -> _GlobalChecked:
    """The refusals of global_registration that do not depend on the clouds, all ValueError."""
    from . import features as F
    g2 = check_parameters(max_distance, who=who).g2
    kk = _integer(k, F.MIN_K, F.MAX_K, f"{who}: k")
    nk = _integer(normals, N.MIN_K, N.MAX_K, f"{who}: normals")
    T = _integer(iterations, 1, MAX_HYPOTHESES, f"{who}: iterations")
    try:
        np.random.default_rng(seed)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: seed={seed!r} is not a seed of np.random.default_rng") from None
    try:
        es = float(edge_similarity)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: edge_similarity={edge_similarity!r} must be a number in [0, 1]") from None
    if isinstance(edge_similarity, bool) or not 0.0 <= es <= 1.0:
        raise ValueError(f"{who}: edge_similarity={edge_similarity!r} must be a number in [0, 1]")
    es32 = _F32(es)
    return _GlobalChecked(g2, kk, nk, T, seed, es32 * es32)


def check_global_triples(triples, C, chk: _GlobalChecked, who="global_registration"):
    """(T, 3) int64 triples: the caller's, checked, or the draw of the contract."""
    if triples is None:
        return np.random.default_rng(chk.seed).integers(0, C, size=(chk.T, 3), dtype=np.int64)
    tri = np.asarray(triples)
    if tri.ndim != 2 or tri.shape[1] != 3 or not 1 <= tri.shape[0] <= MAX_HYPOTHESES or tri.dtype.kind not in "iu":
        raise ValueError(f"{who}: triples have shape {tuple(tri.shape)} and dtype {tri.dtype}, expected (T, 3) integers with "
                         f"1 <= T <= {MAX_HYPOTHESES}")
    if (tri < 0).any() or (tri >= C).any():
        raise ValueError(f"{who}: triples hold an index outside [0, {C})")
    return np.ascontiguousarray(tri.astype(np.int64))


def _sq(e):
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]


def _cross3(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _triangle(p0, p1, p2):
    """(edge lengths squared (3), u, v, w) of the contract for (T, 3) float32 corner arrays; components as tuples of (T,)."""
    c0, c1, c2 = (tuple(p[:, a] for a in range(3)) for p in (p0, p1, p2))
    e1 = tuple(c1[a] - c0[a] for a in range(3))
    e2 = tuple(c2[a] - c0[a] for a in range(3))
    e3 = tuple(c2[a] - c1[a] for a in range(3))
    ls = (_sq(e1), _sq(e2), _sq(e3))
    r = np.sqrt(ls[0])
    u = tuple(e / r for e in e1)
    c = _cross3(e1, e2)
    rc = np.sqrt(_sq(c))
    w = tuple(x / rc for x in c)
    return ls, u, _cross3(w, u), w


def global_hypotheses_host(src, tgt, corr, tri, s2):
    """(T, 12) float32: R row-major then t of every triple, twelve NaNs for an invalid one."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        a = [src[tri[:, m]] for m in range(3)]
        b = [tgt[corr[tri[:, m]]] for m in range(3)]
        la, ua, va, wa = _triangle(*a)
        lb, ub, vb, wb = _triangle(*b)
        valid = np.ones(tri.shape[0], bool)
        for x, y in zip(la, lb):
            valid &= (x > 0) & (y > 0) & (x >= s2 * y) & (y >= s2 * x)
        hyp = np.empty((tri.shape[0], 12), _F32)
        for r in range(3):
            for s in range(3):
                hyp[:, 3 * r + s] = (ub[r] * ua[s] + vb[r] * va[s]) + wb[r] * wa[s]
        a0, b0 = a[0], b[0]
        for r in range(3):
            hyp[:, 9 + r] = b0[:, r] - ((hyp[:, 3 * r] * a0[:, 0] + hyp[:, 3 * r + 1] * a0[:, 1]) + hyp[:, 3 * r + 2] * a0[:, 2])
    valid &= np.isfinite(hyp).all(axis=1)
    hyp[~valid] = np.nan
    return hyp


def global_inliers_host(src, b, hyp, g2):
    """(P, C) bool: the score rule for every row of hyp (P, 12) float32; b = target[correspondence]."""
    h = hyp[:, :, None]
    x, y, z = src[None, :, 0], src[None, :, 1], src[None, :, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        e = [(((h[:, 3 * r] * x + h[:, 3 * r + 1] * y) + h[:, 3 * r + 2] * z) + h[:, 9 + r]) - b[None, :, r] for r in range(3)]
        e2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        assert e2.dtype == _F32
        return e2 <= g2


def global_counts_host(src, b, hyp, g2):
    """(T,) int32: the inliers of every hypothesis (the NaN rows count 0 and are not evaluated)."""
    counts = np.zeros(hyp.shape[0], np.int64)
    rows = np.flatnonzero(~np.isnan(hyp[:, 0]))
    C = src.shape[0]
    cstep = min(C, _SCORE_BLOCK)
    tstep = max(1, _SCORE_BLOCK // cstep)
    for j in range(0, C, cstep):
        for t in range(0, rows.shape[0], tstep):
            sel = rows[t:t + tstep]
            counts[sel] += global_inliers_host(src[j:j + cstep], b[j:j + cstep], hyp[sel], g2).sum(axis=1)
    return counts.astype(np.int32)


def hypothesis_matrix(row):
    """(4, 4) float64 from the twelve float32 entries of a hypothesis."""
    T = np.eye(4)
    T[:3, :3] = np.asarray(row[:9], np.float64).reshape(3, 3)
    T[:3, 3] = np.asarray(row[9:12], np.float64)
    return T


def global_sums_host(src, b, T, g2):
    """(sums (16,) float64, inlier (C,) bool) of the transform T (4, 4) float64 by the score rule and the sums rule."""
    row = np.concatenate((T[:3, :3].astype(_F32).ravel(), T[:3, 3].astype(_F32)))[None]
    inlier = global_inliers_host(src, b, row, g2)[0]
    a64, b64 = src.astype(np.float64), b.astype(np.float64)
    cols = np.concatenate((np.ones((src.shape[0], 1)), a64, b64, (a64[:, :, None] * b64[:, None, :]).reshape(-1, 9)), axis=1)
    cols = np.where(inlier[:, None], cols, 0.0)
    return B.fixed_sums(cols, np.array([src.shape[0]]))[0], inlier


def kabsch(sums):
    """The refinement of the contract from the sixteen sums: (4, 4) float64, or None when there is none."""
    s = np.asarray(sums, np.float64)
    n, Sa, Sb, Sab = s[0], s[1:4], s[4:7], s[7:16].reshape(3, 3)
    try:
        with np.errstate(all="ignore"):
            H = Sab - np.outer(Sa, Sb) / n
            U, _, Vt = np.linalg.svd(H)
            D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(Vt.T @ U.T) >= 0.0 else -1.0])
            R = Vt.T @ D @ U.T
            T = np.eye(4)
            T[:3, :3] = R
            T[:3, 3] = Sb / n - R @ (Sa / n)
    except np.linalg.LinAlgError:
        return None
    return T if np.isfinite(T).all() else None


def global_run(hyp_counts, sums_of, C):
    """The decision part of the contract, what the twin and the device path both call: hyp_counts() -> (hypotheses (T, 12)
    float32, counts (T,) int32) as numpy arrays; sums_of(T (4, 4) float64) -> (sums (16,) float64, inlier (C,) bool or a
    device tensor).  Returns (transformation, count, inlier, best, counts, hypotheses, sums, status)."""
    hyp, counts = hyp_counts()
    best = int(np.argmax(counts))                   # the first maximum
    if counts[best] == 0:
        return np.eye(4), 0, None, -1, counts, hyp, np.zeros(SUM_COLUMNS), "not_found"
    T, status = hypothesis_matrix(hyp[best]), "hypothesis"
    sums, inlier = sums_of(T)
    count = int(sums[0])
    if count >= 3:
        K = kabsch(sums)
        if K is not None:
            T, status = K, "refined"
            final, inlier = sums_of(T)
            count = int(final[0])
    return T, count, inlier, best, counts, hyp, sums, status


def _global_checked_host(src, tgt, corr, tri, chk: _GlobalChecked) -> GlobalRegistrationResult:
    C = src.shape[0]
    b = np.ascontiguousarray(tgt[corr])

    def hyp_counts():
        hyp = global_hypotheses_host(src, tgt, corr, tri, chk.s2)
        return hyp, global_counts_host(src, b, hyp, chk.g2)

    T, count, inlier, best, counts, hyp, sums, status = global_run(hyp_counts, lambda M: global_sums_host(src, b, M, chk.g2), C)
    inlier = np.zeros(C, bool) if inlier is None else inlier
    return GlobalRegistrationResult(T, count, count / C, inlier, corr, best, counts, hyp, sums, status)


def _global_clouds(source, target, source_normals, target_normals, source_viewpoint, target_viewpoint, chk, who):
    """The refusals of the two clouds: features.check_inputs of each, and C >= 3."""
    from . import features as F
    s = F.check_inputs(_host_array(source), chk.k, None if source_normals is None else _host_array(source_normals), chk.normals,
                       source_viewpoint, who, "source")
    t = F.check_inputs(_host_array(target), chk.k, None if target_normals is None else _host_array(target_normals), chk.normals,
                       target_viewpoint, who, "target")
    return s, t                                     # (k >= 2: every cloud has at least 3 points)


def global_registration_host(source, target, *, max_distance, k=30, normals=16, iterations=65536, seed=0, edge_similarity=0.9,
                             source_viewpoint=None, target_viewpoint=None, source_normals=None, target_normals=None,
                             triples=None) -> GlobalRegistrationResult:
    """The numpy twin of the device global registration; see the module docstring for the contract."""
    from . import features as F
    who = "global_registration"
    chk = check_global_parameters(max_distance, k, normals, iterations, seed, edge_similarity, who)
    s, t = _global_clouds(source, target, source_normals, target_normals, source_viewpoint, target_viewpoint, chk, who)
    tri = check_global_triples(triples, s[0].shape[0], chk, who)
    corr, _ = F._match_checked_host(F._fpfh_checked_host(*s).code, F._fpfh_checked_host(*t).code)
    return _global_checked_host(s[0], t[0], corr, tri, chk)


def global_registration_device(s, t, tri, chk: _GlobalChecked, device) -> GlobalRegistrationResult:
    """global_registration of checked arguments (s, t: features.check_inputs of the two clouds, whose points and normals may
    be float32 tensors on `device`) on a cuda device; `inlier` and `correspondence` of the result are device tensors."""
    import torch
    from . import features as F
    from .. import _ops as ops
    with torch.cuda.device(device), torch.no_grad():
        _, code_s, _, _ = F.fpfh_device(*s, device)
        _, code_t, _, _ = F.fpfh_device(*t, device)
        corr, _ = ops.match_features(code_s, code_t)
        src = (s[0] if torch.is_tensor(s[0]) else torch.from_numpy(s[0])).to(device)
        tgt = (t[0] if torch.is_tensor(t[0]) else torch.from_numpy(t[0])).to(device)
        C = src.shape[0]
        T, count, inlier, best, counts, hyp, sums, status = ops.global_ransac(src, tgt, corr, tri, float(chk.s2), float(chk.g2))
        inlier = torch.zeros(C, dtype=torch.bool, device=src.device) if inlier is None else inlier
        return GlobalRegistrationResult(T, count, count / C, inlier, corr, best, counts, hyp, sums, status)


def global_registration(source, target, *, max_distance, k=30, normals=16, iterations=65536, seed=0, edge_similarity=0.9,
                        source_viewpoint=None, target_viewpoint=None, source_normals=None, target_normals=None, triples=None,
                        device=None) -> GlobalRegistrationResult:
    """The rigid transform that moves `source` (Ms, 3) onto `target` (Mt, 3) without an initial pose, from FPFH
    correspondences and RANSAC over them: GlobalRegistrationResult(transformation, count, fitness, inlier, correspondence,
    best, counts, hypotheses, sums, status) - see the module docstring.  What icp(init=...) starts from.  Runs on the GPU
    (rl_knn_f32, rl_normals, csrc/fpfh.hip, csrc/match.hip, csrc/global.hip; Kabsch on the host) when `device` is a cuda
    device, or when it is None and one is available; otherwise global_registration_host.  The clouds may be float32 tensors
    on that device.  Either way the result is numpy arrays, and the same ones bit for bit."""
    dev = _cuda(device, source, target)
    if dev is None:
        return global_registration_host(source, target, max_distance=max_distance, k=k, normals=normals, iterations=iterations,
                                        seed=seed, edge_similarity=edge_similarity, source_viewpoint=source_viewpoint,
                                        target_viewpoint=target_viewpoint, source_normals=source_normals,
                                        target_normals=target_normals, triples=triples)
    who = "global_registration"
    chk = check_global_parameters(max_distance, k, normals, iterations, seed, edge_similarity, who)
    s, t = _global_clouds(source, target, source_normals, target_normals, source_viewpoint, target_viewpoint, chk, who)
    tri = check_global_triples(triples, s[0].shape[0], chk, who)
    res = global_registration_device(s, t, tri, chk, dev)
    return res._replace(inlier=res.inlier.cpu().numpy(), correspondence=res.correspondence.cpu().numpy())


# ---------------------------------------------------------------------------- Model.predict_views(global_init=...)
_GlobalViews = namedtuple("_GlobalViews", ["cell", "chk", "viewpoints"])


def check_global_settings(settings: GlobalSettings, V: int, who="predict_views") -> _GlobalViews:
    """The refusals of a GlobalSettings for V views, all ValueError: (voxel as float32, the checked parameters, the (V, 3)
    float64 viewpoints)."""
    try:
        cell = _F32(float(settings.voxel))
    except (TypeError, ValueError):
        raise ValueError(f"{who}: global_init.voxel={settings.voxel!r} must be a finite number > 0") from None
    if isinstance(settings.voxel, bool) or not np.isfinite(cell) or not cell > 0:
        raise ValueError(f"{who}: global_init.voxel={settings.voxel!r} must be a finite number > 0")
    md = 1.5 * float(settings.voxel) if settings.max_distance is None else settings.max_distance
    chk = check_global_parameters(md, settings.k, settings.normals, settings.iterations, settings.seed, settings.edge_similarity,
                                  f"{who}: global_init")
    if settings.viewpoints is None:
        vps = np.zeros((V, 3))
    else:
        try:
            vps = np.array(settings.viewpoints, dtype=np.float64)
        except (TypeError, ValueError):
            vps = np.zeros(0)
        if vps.shape != (V, 3) or not np.isfinite(vps).all():
            raise ValueError(f"{who}: global_init.viewpoints must be {V} finite (3,) positions, one per view")
    return _GlobalViews(cell, chk, vps)


def global_between(source, target, v, w, Tw, g: _GlobalViews, thin, device) -> GlobalRegistrationResult:
    """The global registration of view v (`source`) onto `target` - view w moved by Tw (4, 4) - for Model.predict_views:
    both grid-subsampled with g.cell (`thin` caches view 0's, the target of every view with to="first"), the target's
    viewpoint carried into its frame.  numpy clouds and device None: the twins; device tensors: on `device`."""
    from . import features as F
    from . import grid as G
    who = "predict_views: global_init"

    def subsample(cloud):
        if device is None:
            return G.grid_subsample_host(cloud, cell=g.cell).xyz
        import torch
        from .. import _ops as ops
        with torch.cuda.device(device), torch.no_grad():
            return ops.grid_subsample(cloud, None, float(g.cell))[0]

    sub_s = subsample(source)
    if w == 0:
        if 0 not in thin:
            thin[0] = subsample(target)
        sub_t = thin[0]
    else:
        sub_t = subsample(target)
    vp_t = Tw[:3, :3] @ g.viewpoints[w] + Tw[:3, 3]
    C = sub_s.shape[0]
    if device is None:
        s = F.check_inputs(sub_s, g.chk.k, None, g.chk.normals, g.viewpoints[v], who, f"views[{v}], subsampled,")
        t = F.check_inputs(sub_t, g.chk.k, None, g.chk.normals, vp_t, who, f"views[{w}], subsampled,")
        corr, _ = F._match_checked_host(F._fpfh_checked_host(*s).code, F._fpfh_checked_host(*t).code)
        return _global_checked_host(s[0], t[0], corr, check_global_triples(None, C, g.chk, who), g.chk)

    def checked(cloud, viewpoint, u):               # (a subsampled cloud of finite points is finite: only its size can be wrong)
        need = max(g.chk.k + 1, g.chk.normals)
        if cloud.shape[0] < need:
            raise ValueError(f"{who}: views[{u}], subsampled, has M={cloud.shape[0]} points, fewer than the {need} that k and "
                             f"normals need: the voxel is too large")
        return cloud, g.chk.k, None, g.chk.normals, np.ascontiguousarray(np.asarray(viewpoint, np.float64).astype(_F32))

    res = global_registration_device(checked(sub_s, g.viewpoints[v], v), checked(sub_t, vp_t, w),
                                     check_global_triples(None, C, g.chk, who), g.chk, device)
    return res._replace(inlier=res.inlier.cpu().numpy(), correspondence=res.correspondence.cpu().numpy())
