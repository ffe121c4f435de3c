#!/usr/bin/env python3
"""Euclidean clustering (randlanet/utils/cluster.py, csrc/cluster.hip) on one MI355X.  Scenes:
  uniform M   M = 10^6 and 10^7 uniform points in a 40 x 40 x 4 m box, r chosen for about ten neighbours within r; the lowest
              0.4 m are class 0 (ignored), above it the class changes every 2 m in x and y (12 classes), so the instances are
              columns of the box
  chain       one adversarial component: 10^6 points spaced 0.9 r along a serpentine path (rows of 1000 steps, 3.6 r apart,
              joined at alternate ends), the indices a random permutation
Per scene:
  cells / union / reduce   device events around each entry point on points and labels already in HBM, median [min, max] in ms
                           over REPS repetitions after warm-up (the two read-backs are outside these windows)
  device_ms                their sum: the kernels of one clustering
  call_s                   the public euclidean_clusters(device="cuda") on numpy input: upload, kernels, two read-backs, download
  twin_s                   euclidean_clusters_host on the same input (numpy, this machine's CPUs), scenes up to --twin-max points
Prints one JSON line.  Not part of bench.py, not run by any test.
usage: python tools/time_clusters.py [--sizes 1000000,10000000] [--chain 1000000] [--twin-max 10000000]"""
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
from randlanet.utils import cluster as K  # noqa: E402

BOX = np.array([40.0, 40.0, 4.0])
REPS, WARM = 5, 2


def uniform_scene(M: int, neighbours: float = 10.0):
    rs = np.random.RandomState(M % 9973)
    xyz = (rs.rand(M, 3) * BOX).astype(np.float32)
    labels = 1 + (np.floor(xyz[:, 0] / 2) + 5 * np.floor(xyz[:, 1] / 2)).astype(np.int64) % 12
    labels[xyz[:, 2] < 0.4] = 0
    r = float((neighbours * BOX.prod() / M / (4.0 / 3.0 * np.pi)) ** (1.0 / 3.0))
    return xyz, labels, round(r, 4), rs.rand(M).astype(np.float32)


def chain_scene(M: int):
    rs = np.random.RandomState(7)
    r = 0.05
    k = np.arange(M - 1)
    row, along = k // 1004, k % 1004 < 1000
    step = np.stack([np.where(along, np.where(row % 2 == 0, 1.0, -1.0), 0.0), np.where(along, 0.0, 1.0)], axis=1)
    xy = np.concatenate([np.zeros((1, 2)), np.cumsum(step, axis=0)]) * (0.9 * r)
    xyz = np.concatenate([xy, np.full((M, 1), 1.0)], axis=1).astype(np.float32)[rs.permutation(M)]
    return xyz, np.ones(M, np.int64), r, rs.rand(M).astype(np.float32)


def spread(v):
    return {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def device_phases(xyz_d, labels_d, scores_d, r, ignore_d):
    lib, dev = H.lib(), xyz_d.device
    M = xyz_d.shape[0]
    ws = ops.cluster_workspace(dev, M)
    head = torch.empty(4, dtype=torch.int64, device=dev)
    instance = torch.empty(M, dtype=torch.int32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    st = H.stream_ptr
    ev[0].record()
    H.check(lib.rl_cluster_cells(xyz_d.data_ptr(), M, r, head.data_ptr(), ws.data_ptr(), ws.numel(), st()))
    ev[1].record()
    dims = head[:3].tolist()
    K.check_dims(dims)
    ev[2].record()
    H.check(lib.rl_cluster_union(xyz_d.data_ptr(), labels_d.data_ptr(), M, r, ignore_d.data_ptr(), ignore_d.numel(),
                                 K.key_bits(dims), 1, instance.data_ptr(), head[3:].data_ptr(), ws.data_ptr(), ws.numel(), st()))
    ev[3].record()
    I = int(head[3].item())
    out = [torch.empty(I, dtype=torch.int64, device=dev), torch.empty(I, dtype=torch.int32, device=dev)]
    out += [torch.empty((I, 3), dtype=torch.float32, device=dev) for _ in range(3)]
    out.append(torch.empty(I, dtype=torch.float32, device=dev))
    ev[4].record()
    H.check(lib.rl_cluster_reduce(xyz_d.data_ptr(), labels_d.data_ptr(), scores_d.data_ptr(), M, I,
                                  *(t.data_ptr() for t in out), ws.data_ptr(), ws.numel(), st()))
    ev[5].record()
    torch.cuda.synchronize()
    return {"cells": ev[0].elapsed_time(ev[1]), "union": ev[2].elapsed_time(ev[3]), "reduce": ev[4].elapsed_time(ev[5])}, I, dims


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--chain", type=int, default=1000000)
    ap.add_argument("--twin-max", type=int, default=10000000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_clusters measures the MI355X"
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "reps": REPS, "rows": []}
    scenes = [(f"uniform {int(s)}", uniform_scene(int(s))) for s in args.sizes.split(",") if s]
    if args.chain:
        scenes.append((f"chain {args.chain}", chain_scene(args.chain)))
    for name, (xyz, labels, r, scores) in scenes:
        M = xyz.shape[0]
        with torch.cuda.device(dev), torch.no_grad():
            xyz_d, labels_d, scores_d = (torch.from_numpy(a).to(dev) for a in (xyz, labels, scores))
            ignore_d = torch.zeros(1, dtype=torch.int64, device=dev)
            runs = [device_phases(xyz_d, labels_d, scores_d, float(np.float32(r)), ignore_d) for _ in range(WARM + REPS)]
            del xyz_d, labels_d, scores_d
            torch.cuda.empty_cache()
        timed = [t[0] for t in runs[WARM:]]
        calls = []
        for _ in range(1 + 3):
            t0 = time.perf_counter()
            got = K.euclidean_clusters(xyz, labels, radius=r, scores=scores, device=dev)
            calls.append(time.perf_counter() - t0)
        row = {"scene": name, "M": M, "radius": r, "dims": runs[-1][2], "instances": runs[-1][1],
               "largest": int(got.count.max()) if got.count.size else 0}
        for ph in ("cells", "union", "reduce"):
            row[ph + "_ms"] = spread([t[ph] for t in timed])
        row["device_ms"] = spread([sum(t.values()) for t in timed])
        row["call_s"] = spread(calls[1:])
        if M <= args.twin_max:
            t0 = time.perf_counter()
            ref = K.euclidean_clusters_host(xyz, labels, radius=r, scores=scores)
            row["twin_s"] = round(time.perf_counter() - t0, 3)
            row["equals_twin"] = all(np.array_equal(a, b) for a, b in zip(got, ref))
        res["rows"].append(row)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
