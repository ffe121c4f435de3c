#!/usr/bin/env python3
"""Rigid registration by ICP (randlanet/utils/registration.py, csrc/icp.hip) on one MI355X.  Clouds: a room corner - a bumpy
floor, two walls and a dome, sized so that the density stays at 250000 points per square unit - as the target, and as the
source the same number of other samples of it, moved by 2 degrees and a shift of four point spacings; Ms = Mt = 150000, 501221
(a 1024 x 768 camera frame after the range gate) and 10^6, max_distance = ten point spacings.  Per size and metric:
  transform_ms / knn_ms / sums_ms / fold_ms   device events around rl_icp_transform, rl_knn_f32 (B = 1, k = 1, its grid built
                        again over the unchanged target), rl_icp_sums and rl_icp_fold of ONE evaluation on clouds already in
                        HBM; median [min, max] in ms over REPS passes after WARM warm-ups
  knn_share             knn_ms over the sum of the four: what a K-NN that builds its grid once could save is inside it
  icp_ms                the whole _ops.icp on the device clouds (the target's normals given) - every evaluation with its
                        read-back of 30 doubles and the host's 6x6 solve -, wall clock; evaluations = updates + 1
  normals_ms            _ops.estimate_normals of the target (k = 16), which icp runs first when no normals are given
  twin_s                icp_host on the same input (numpy, this machine's CPUs), up to --twin-max points; equals_twin: every
                        field bit for bit
Prints one JSON line.  Not part of bench.py, not run by any test.
usage: python tools/time_registration.py [--sizes 150000,501221,1000000] [--twin-max 150000]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "3d_recognizer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from randlanet import _hip as H  # noqa: E402
from randlanet import _ops as ops  # noqa: E402
from randlanet.utils import registration as R  # noqa: E402

REPS, WARM = 5, 2
ITERATIONS = 30


def corner(M: int, seed: int) -> np.ndarray:
    """M samples of the corner: three faces of side s and a dome of radius 0.2 s, s^2 * 3.25 * 250000 = M."""
    rs = np.random.RandomState(seed)
    s = np.sqrt(M / (3.25 * 250000.0))
    n = M // 13 * 4
    u = rs.uniform(0, s, (n, 2))
    floor = np.concatenate([u, (0.02 * s * np.sin(6 * u[:, 0] / s) * np.cos(5 * u[:, 1] / s))[:, None]], axis=1)
    v = rs.uniform(0, s, (n, 2))
    wall_x = np.stack((np.zeros(n), v[:, 0], v[:, 1]), axis=1)
    v = rs.uniform(0, s, (n, 2))
    wall_y = np.stack((v[:, 0], np.zeros(n), v[:, 1]), axis=1)
    d = rs.normal(size=(M - 3 * n, 3))
    d[:, 2] = np.abs(d[:, 2])
    dome = np.array([0.55 * s, 0.5 * s, 0.0]) + 0.2 * s * d / np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([floor, wall_x, wall_y, dome])[rs.permutation(M)]


def moved_back(xyz: np.ndarray, degrees: float, shift) -> np.ndarray:
    a, t = np.array([1.0, 2.0, 2.0]) / 3.0, np.radians(degrees)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    Rm = np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)
    return (xyz - np.asarray(shift)) @ Rm


def spread(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def one_evaluation(src, tgt, nrm, gate2, metric):
    """The four entries of one evaluation at T = I with an event pair around each; ms."""
    lib, dev, Ms, Mt = H.lib(), src.device, src.shape[0], tgt.shape[0]
    q = torch.empty_like(src)
    idx = torch.empty((Ms, 1), dtype=torch.int64, device=dev)
    d2 = torch.empty((Ms, 1), dtype=torch.float32, device=dev)
    corr = torch.empty(Ms, dtype=torch.int64, device=dev)
    out = torch.empty(30, dtype=torch.float64, device=dev)
    ws = ops.icp_workspace(dev, Ms)
    kws, kbytes = ops._knn_workspace(dev, 1, Mt, Ms, 1, False)
    rt = ops._icp_rt(np.eye(4))
    e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    st = H.stream_ptr()
    e[0].record()
    H.check(lib.rl_icp_transform(src.data_ptr(), Ms, 0, Ms, rt, q.data_ptr(), st))
    e[1].record()
    H.check(lib.rl_knn_f32(tgt.data_ptr(), q.data_ptr(), 1, Mt, Ms, 1, idx.data_ptr(), d2.data_ptr(), H.ptr(kws), kbytes, st))
    e[2].record()
    H.check(lib.rl_icp_sums(q.data_ptr(), H.ptr(nrm), tgt.data_ptr(), Mt, idx.data_ptr(), d2.data_ptr(), Ms, 0, Ms, gate2, metric,
                            corr.data_ptr(), ws.data_ptr(), ws.numel(), st))
    e[3].record()
    H.check(lib.rl_icp_fold(Ms, out.data_ptr(), ws.data_ptr(), ws.numel(), st))
    e[4].record()
    torch.cuda.synchronize()
    return [e[j].elapsed_time(e[j + 1]) for j in range(4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="150000,501221,1000000")
    ap.add_argument("--twin-max", type=int, default=150000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_registration measures the MI355X"
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "reps": REPS, "iterations": ITERATIONS, "rows": []}
    for M in (int(s) for s in args.sizes.split(",") if s):
        spacing = 0.002
        tgt_h = corner(M, 1).astype(np.float32)
        src_h = moved_back(corner(M, 2), 2.0, (4 * spacing, -3 * spacing, 2 * spacing)).astype(np.float32)
        with torch.cuda.device(dev), torch.no_grad():
            src, tgt = torch.from_numpy(src_h).to(dev), torch.from_numpy(tgt_h).to(dev)
            nrm_t = []
            for _ in range(WARM + REPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                nrm = ops.estimate_normals(tgt, 16)[0]
                torch.cuda.synchronize()
                nrm_t.append(1e3 * (time.perf_counter() - t0))
            for metric in R.METRICS:
                chk = R.check_parameters(10 * spacing, metric=metric, iterations=ITERATIONS)
                n = nrm if chk.metric == 0 else None
                runs = [one_evaluation(src, tgt, n, float(chk.g2), chk.metric) for _ in range(WARM + REPS)][WARM:]
                cols = [[r[j] for r in runs] for j in range(4)]
                walls = []
                for _ in range(WARM + REPS):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got = ops.icp(src, tgt, n, chk)
                    torch.cuda.synchronize()
                    walls.append(1e3 * (time.perf_counter() - t0))
                med = [float(np.median(c)) for c in cols]
                row = {"M": M, "metric": metric, "workspace_bytes": int(H.lib().rl_icp_workspace_bytes(M)),
                       "transform_ms": spread(cols[0]), "knn_ms": spread(cols[1]), "sums_ms": spread(cols[2]),
                       "fold_ms": spread(cols[3]), "knn_share": round(med[1] / sum(med), 3), "icp_ms": spread(walls[WARM:]),
                       "evaluations": int(got[4]) + 1, "status": got[5], "fitness": round(got[1], 4),
                       "inlier_rmse": float(f"{got[2]:.4g}"), "normals_ms": spread(nrm_t[WARM:])}
                if M <= args.twin_max:
                    t0 = time.perf_counter()
                    ref = R.icp_host(src_h, tgt_h, max_distance=10 * spacing, metric=metric, iterations=ITERATIONS,
                                     target_normals=None if n is None else n.cpu().numpy())
                    row["twin_s"] = round(time.perf_counter() - t0, 3)
                    row["equals_twin"] = bool(np.array_equal(got[0], ref.transformation) and np.array_equal(got[7], ref.history)
                                              and np.array_equal(got[6].cpu().numpy(), ref.correspondence)
                                              and np.array_equal(got[8].cpu().numpy(), ref.transformed))
                res["rows"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
            del src, tgt, nrm
    print(json.dumps(res))


if __name__ == "__main__":
    main()
