#!/usr/bin/env python3
"""Grid subsampling (randlanet/utils/grid.py, csrc/grid.hip) on one MI355X: scenes of M = 10^6 and 10^7 uniform points in a
40 x 40 x 4 m box with F = 3 features and labels over 13 classes, the cell chosen for about ten points per cell.  Per M:
  bounds / sort / heads / reduce   device events around each entry point on a cloud already in HBM, median [min, max] in ms
                                   over REPS repetitions after warm-up (the two read-backs are outside these windows)
  device_ms                        their sum: the kernels of one subsampling
  call_s                           the public grid_subsample(device="cuda") on numpy input: upload, kernels, two read-backs,
                                   download of the result - what a caller with host arrays pays
  twin_s                           grid_subsample_host on the same input (numpy, this machine's CPUs), the yardstick
  confusion_ms                     rl_scene_confusion over the M raw points (13 classes, through inverse)
and for M = 10^7, a config-S-shaped network (13 classes, K = 16, n = 40960, B = 8): predict_scene(votes=1) without and with
grid - crops, passes, seconds.  Prints one JSON line.  Not part of bench.py.
usage: python tools/grid_bench.py [--sizes 1000000,10000000] [--no-predict]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "3d_recognizer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from randlanet import Model, RandLANetSettings  # noqa: E402
from randlanet import _hip as H  # noqa: E402
from randlanet import _ops as ops  # noqa: E402
from randlanet.utils import grid  # noqa: E402

N, B, C, F = 40960, 8, 13, 3
BOX = np.array([40.0, 40.0, 4.0])
REPS, WARM = 7, 2


def cell_for(M: int, per_cell: float = 10.0) -> float:
    return round(float((BOX.prod() * per_cell / M) ** (1.0 / 3.0)), 4)


def phase_bytes(M: int, V: int, dim: int, passes: int) -> dict:
    """Bytes each phase must move: bounds reads whole rows; a sort pass reads the keys twice (histogram, scatter) and the
    indices once and writes both; heads read the keys twice and the indices once, write inverse and the starts; the
    reduction gathers M rows (and M labels per class it counts) and writes V rows."""
    return {"bounds": 4 * dim * M, "sort": 4 * dim * M + 8 * M + passes * (8 + 8 + 4 + 8 + 4) * M - 4 * M,
            "heads": (8 + 8 + 4 + 4) * M + 4 * V, "reduce": (4 * dim + 4 + 8) * M + V * (4 * dim + 4 + 8 + 8)}


def spread(ms):
    return {"median": round(float(np.median(ms)), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def device_phases(cloud_d, labels_d, cell):
    """One subsampling through the entry points, each under its own pair of events.  Returns ({phase: ms}, V, key bits)."""
    lib, dev = H.lib(), cloud_d.device
    M, dim = cloud_d.shape
    ws = ops.grid_workspace(dev, M, dim)
    head = torch.empty(4, dtype=torch.int64, device=dev)
    inverse = torch.empty(M, dtype=torch.int32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
    st = H.stream_ptr
    ev[0].record()
    H.check(lib.rl_grid_bounds(cloud_d.data_ptr(), M, dim, cell, head.data_ptr(), ws.data_ptr(), ws.numel(), st()))
    ev[1].record()
    dims = head[:3].tolist()
    bits = grid.key_bits(dims)
    ev[2].record()
    H.check(lib.rl_grid_sort(cloud_d.data_ptr(), M, dim, bits, ws.data_ptr(), ws.numel(), st()))
    ev[3].record()
    H.check(lib.rl_grid_heads(M, dim, head[3:].data_ptr(), inverse.data_ptr(), ws.data_ptr(), ws.numel(), st()))
    ev[4].record()
    V = int(head[3].item())
    rows = torch.empty((V, dim), dtype=torch.float32, device=dev)
    count = torch.empty(V, dtype=torch.int32, device=dev)
    lab = torch.empty(V, dtype=torch.int64, device=dev)
    ev[5].record()
    H.check(lib.rl_grid_reduce(cloud_d.data_ptr(), M, dim, labels_d.data_ptr(), C, V, rows.data_ptr(), lab.data_ptr(),
                               count.data_ptr(), ws.data_ptr(), ws.numel(), st()))
    ev[6].record()
    torch.cuda.synchronize()
    return ({"bounds": ev[0].elapsed_time(ev[1]), "sort": ev[2].elapsed_time(ev[3]), "heads": ev[3].elapsed_time(ev[4]),
             "reduce": ev[5].elapsed_time(ev[6])}, V, bits, inverse)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--no-predict", action="store_true")
    ap.add_argument("--twin-reps", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "grid_bench measures the MI355X"
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "features": F, "classes": C, "reps": REPS, "rows": []}
    for M in [int(s) for s in args.sizes.split(",")]:
        rs = np.random.RandomState(M % 9973)
        xyz = (rs.rand(M, 3) * BOX).astype(np.float32)
        feats = rs.rand(M, F).astype(np.float32)
        labels = rs.randint(0, C, M).astype(np.int64)
        cell = cell_for(M)
        with torch.cuda.device(dev), torch.no_grad():
            cloud_d = torch.from_numpy(np.concatenate((xyz, feats), axis=1)).to(dev)
            labels_d = torch.from_numpy(labels).to(dev)
            runs = [device_phases(cloud_d, labels_d, cell) for _ in range(WARM + REPS)]
            phases, V, bits, inverse = runs[-1]
            timed = [r[0] for r in runs[WARM:]]
            prob = torch.rand((V, C), dtype=torch.float32, device=dev)
            table = torch.zeros((C, C), dtype=torch.int64, device=dev)
            conf = []
            for _ in range(WARM + REPS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.scene_confusion(prob, labels_d, table, inverse)
                e1.record()
                torch.cuda.synchronize()
                conf.append(e0.elapsed_time(e1))
            del cloud_d, labels_d, prob, inverse, runs
            torch.cuda.empty_cache()
        calls = []
        for _ in range(1 + 3):
            t0 = time.perf_counter()
            got = grid.grid_subsample(xyz, feats, labels, cell=cell, n_classes=C, device=dev)
            calls.append(time.perf_counter() - t0)
        twins = []
        for _ in range(args.twin_reps):
            t0 = time.perf_counter()
            ref = grid.grid_subsample_host(xyz, feats, labels, cell=cell, n_classes=C)
            twins.append(time.perf_counter() - t0)
        same = all(np.array_equal(a, b) for a, b in zip(got, ref))
        passes = (bits + 7) // 8
        nb = phase_bytes(M, V, 3 + F, passes)
        row = {"M": M, "cell": cell, "V": V, "points_per_cell": round(M / V, 2), "key_bits": bits, "sort_passes": passes,
               "equals_twin": bool(same)}
        for ph in ("bounds", "sort", "heads", "reduce"):
            row[ph + "_ms"] = spread([t[ph] for t in timed])
            row[ph + "_GBps"] = round(nb[ph] / (row[ph + "_ms"]["median"] * 1e-3) / 1e9, 1)
        row["device_ms"] = spread([sum(t.values()) for t in timed])
        row["confusion_ms"] = spread(conf[WARM:])
        row["call_s"] = spread(calls[1:])
        row["twin_s"] = spread(twins)
        res["rows"].append(row)
    if not args.no_predict:
        M = 10 ** 7
        torch.manual_seed(0)
        model = Model(RandLANetSettings(n_classes=C, n_points=N, n_neighbors=16, layer_sizes=[16, 64, 128, 256, 512]))
        rs = np.random.RandomState(M % 9973)
        xyz = (rs.rand(M, 3) * BOX).astype(np.float32)
        cell = cell_for(M)
        model.predict_scene(xyz[:200000], batch_size=B)                      # warm both call paths once
        model.predict_scene(xyz[:400000], batch_size=B, grid=cell_for(400000))
        pred = {"M": M, "n": N, "B": B, "cell": cell}
        for name, g in (("raw", None), ("grid", cell)):
            secs = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, counts = model.predict_scene(xyz, batch_size=B, return_counts=True, grid=g)
                secs.append(time.perf_counter() - t0)
            if g is None:
                crops = int(counts.sum()) // N
            else:       # the counts are per raw point: count each representative once
                sub = grid.grid_subsample(xyz, cell=g, device=dev)
                first = np.full(sub.xyz.shape[0], -1, np.int64)
                first[sub.inverse] = np.arange(M)
                crops = int(counts[first].sum()) // N
                pred["V"] = int(sub.xyz.shape[0])
            pred[name] = {"crops": crops, "passes": crops // B, "seconds": spread(secs)}
        res["predict_scene"] = pred
    print(json.dumps(res))


if __name__ == "__main__":
    main()
