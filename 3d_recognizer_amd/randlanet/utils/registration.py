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

Not here: scale estimation; robust kernels; colored or generalised ICP; global (feature-based) initialisation - `init` is
the caller's -; clouds far from the origin: a = p x n is formed in the caller's coordinates, so shift such scans first; a
K-NN that keeps its grid between iterations: every evaluation builds the target's grid again.
"""
from collections import namedtuple
from dataclasses import dataclass

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
