#!/usr/bin/env python3
"""Statistical outlier removal (randlanet/utils/outliers.py, csrc/outliers.hip) on one MI355X.  Clouds: a noisy terrain-like
surface (tools/time_normals.py's) and uniform noise in a cube of the same density per volume, M points each - a depth-camera
frame (150000 points) and a terrestrial scan (10^7) - with k = 16, std_ratio = 2.  Per cloud:
  knn_ms / mean_ms      device events around every rl_knn_f32 (k + 1 rows) and every rl_outliers_mean_distance call of one
                        _ops.statistical_outliers pass over coordinates already in HBM (chunk = 2^20 queries), summed over the
                        chunks; median [min, max] in ms over REPS passes after warm-up
  threshold_ms          rl_outliers_threshold: the two fixed-order sums, mu, sigma and the threshold (4 launches)
  compact_ms            rl_outliers_compact: the mask and the stable compaction (3 launches)
  new_share             (mean_ms + threshold_ms + compact_ms) / knn_ms, from the medians
  call_s                the public statistical_outliers(device="cuda") on numpy input: upload, kernels, download
  twin_s                statistical_outliers_host on the same input (numpy + the host K-NN, this machine's CPUs), up to --twin-max
With --scene: one Model.predict_scene (a small network, votes = 1) of the largest surface cloud with grid=, with and without
outliers=, wall-clock seconds after one warm-up call each.
Prints one JSON line.  Not part of bench.py, not run by any test.
usage: python tools/time_outliers.py [--sizes 150000,10000000] [--k 16] [--std-ratio 2] [--twin-max 150000]
       [--scene [--cell 0.1]]"""
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
from randlanet.utils import outliers as O  # noqa: E402

REPS, WARM = 5, 2
CHUNK = 1 << 20


def surface(M: int) -> np.ndarray:
    rs = np.random.RandomState(M % 9973)
    side = np.sqrt(M / 2500.0)                      # 2500 points per square metre
    u = rs.rand(M, 2) * side
    z = 0.5 * np.sin(0.7 * u[:, 0]) * np.cos(0.5 * u[:, 1]) + 0.002 * rs.randn(M)
    return np.stack([u[:, 0], u[:, 1], z], axis=1).astype(np.float32)


def uniform(M: int) -> np.ndarray:
    rs = np.random.RandomState(M % 9967)
    return (rs.rand(M, 3) * np.cbrt(M / 125000.0)).astype(np.float32)      # 125000 points per cubic metre


def spread(v):
    return {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def one_pass(xyz_d, k, ratio, chunk):
    """The launches of ops.statistical_outliers with an event pair around each phase; returns (knn, mean, threshold, compact)
    in ms and the kept count."""
    lib, dev, M, k1 = H.lib(), xyz_d.device, xyz_d.shape[0], k + 1
    mean = torch.empty(M, dtype=torch.float64, device=dev)
    Qmax = min(chunk, M)
    idx = torch.empty((Qmax, k1), dtype=torch.int64, device=dev)
    d2 = torch.empty((Qmax, k1), dtype=torch.float32, device=dev)
    ev = []
    for first in range(0, M, Qmax):
        Q = min(Qmax, M - first)
        nbytes = lib.rl_knn_workspace_bytes(1, M, Q, k1)
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        H.check(lib.rl_knn_f32(xyz_d.data_ptr(), xyz_d[first:].data_ptr(), 1, M, Q, k1, idx.data_ptr(), d2.data_ptr(),
                               ws.data_ptr() if nbytes > 0 else None, max(nbytes, 0), H.stream_ptr()), "rl_knn_f32")
        e[1].record()
        H.check(lib.rl_outliers_mean_distance(d2.data_ptr(), M, first, Q, k, mean.data_ptr(), H.stream_ptr()),
                "rl_outliers_mean_distance")
        e[2].record()
        ev.append(e)
    keep = torch.empty(M, dtype=torch.uint8, device=dev)
    slot = torch.empty(M, dtype=torch.int32, device=dev)
    kept = torch.empty(M, dtype=torch.int64, device=dev)
    stats = torch.empty(4, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.rl_outliers_workspace_bytes(M), dtype=torch.uint8, device=dev)
    f = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    f[0].record()
    H.check(lib.rl_outliers_threshold(mean.data_ptr(), M, float(ratio), stats.data_ptr(), ws.data_ptr(), ws.numel(),
                                      H.stream_ptr()), "rl_outliers_threshold")
    f[1].record()
    H.check(lib.rl_outliers_compact(mean.data_ptr(), M, keep.data_ptr(), slot.data_ptr(), kept.data_ptr(), stats.data_ptr(),
                                    ws.data_ptr(), ws.numel(), H.stream_ptr()), "rl_outliers_compact")
    f[2].record()
    torch.cuda.synchronize()
    return (sum(e[0].elapsed_time(e[1]) for e in ev), sum(e[1].elapsed_time(e[2]) for e in ev), f[0].elapsed_time(f[1]),
            f[1].elapsed_time(f[2]), int(stats[3].item()))


def scene_times(xyz, k, ratio, cell):
    """Wall-clock seconds of one predict_scene with grid=, without and with outliers= (a small network; after one warm-up)."""
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    model = Model(RandLANetSettings(n_classes=4, n_points=16384, n_neighbors=16, layer_sizes=[16, 32, 64, 128]), use_gpu=True)
    out = {"cell": cell}
    for name, kw in (("plain_s", {}), ("outliers_s", {"outliers": (k, ratio)})):
        t = []
        for _ in range(2):
            np.random.seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = model.predict_scene(xyz, grid=cell, votes=1, batch_size=8, return_outliers=True, **kw)
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        out[name] = round(t[1], 3)
        out[name.replace("_s", "_removed")] = int(res[1].sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="150000,10000000")
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--std-ratio", type=float, default=2.0)
    ap.add_argument("--twin-max", type=int, default=150000)
    ap.add_argument("--scene", action="store_true")
    ap.add_argument("--cell", type=float, default=0.1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_outliers measures the MI355X"
    dev = torch.device("cuda", 0)
    k, ratio = args.k, args.std_ratio
    res = {"device": torch.cuda.get_device_name(0), "reps": REPS, "k": k, "std_ratio": ratio, "chunk": CHUNK, "rows": []}
    sizes = [int(s) for s in args.sizes.split(",") if s]
    for M in sizes:
        for shape, make in (("surface", surface), ("uniform", uniform)):
            xyz = make(M)
            with torch.cuda.device(dev), torch.no_grad():
                xyz_d = torch.from_numpy(xyz).to(dev)
                runs = [one_pass(xyz_d, k, ratio, CHUNK) for _ in range(WARM + REPS)][WARM:]
                del xyz_d
                torch.cuda.empty_cache()
            calls = []
            for _ in range(1 + 3):
                t0 = time.perf_counter()
                got = O.statistical_outliers(xyz, k, ratio, device=dev)
                calls.append(time.perf_counter() - t0)
            cols = [[r[j] for r in runs] for j in range(4)]
            med = [float(np.median(c)) for c in cols]
            row = {"cloud": shape, "M": M, "chunks": -(-M // CHUNK), "kept": runs[0][4], "knn_ms": spread(cols[0]),
                   "mean_ms": spread(cols[1]), "threshold_ms": spread(cols[2]), "compact_ms": spread(cols[3]),
                   "new_share": round(sum(med[1:]) / med[0], 4), "call_s": spread(calls[1:])}
            if M <= args.twin_max:
                t0 = time.perf_counter()
                ref = O.statistical_outliers_host(xyz, k, ratio)
                row["twin_s"] = round(time.perf_counter() - t0, 3)
                row["equals_twin"] = bool(np.array_equal(got.keep, ref.keep) and got.threshold == ref.threshold
                                          and np.array_equal(got.mean_distance.view(np.uint64),
                                                             ref.mean_distance.view(np.uint64)))
            res["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    if args.scene:
        res["predict_scene"] = dict(M=max(sizes), **scene_times(surface(max(sizes)), k, ratio, args.cell))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
