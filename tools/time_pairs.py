#!/usr/bin/env python3
"""Pair counts (randlanet/utils/instance_metrics.py, csrc/pairs.hip) on one MI355X.  Inputs: M points, predicted ids a (int32,
as the clustering writes them) and ground-truth ids b (int64) below `ids`, b equal to a for nine points in ten and random
for the tenth, one point in ten without an instance on either side (-1): the table of an instance evaluation.
Per size:
  sort / write   device events around each entry point on ids already in HBM, median [min, max] in ms over REPS repetitions
                 after warm-up (the read-back of P and the flag is outside these windows)
  device_ms      their sum: the kernels of one table
  ops_ms         _ops.pair_counts on device tensors, host clock to a synchronise: workspace, kernels, the read-back, outputs
  call_ms        the public pair_counts(device="cuda") on numpy input: upload, kernels, read-back, download
  twin_ms        pair_counts_host on the same input (numpy, this machine's CPUs), 3 repetitions
Prints one JSON line.  Not part of bench.py, not run by any test.
usage: python tools/time_pairs.py [--sizes 150000,10000000] [--ids 1000]"""
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
from randlanet.utils import instance_metrics as IM  # noqa: E402

REPS, WARM = 5, 2


def scene(M: int, ids: int):
    rs = np.random.RandomState(M % 9973)
    a = rs.randint(0, ids, M)
    b = np.where(rs.rand(M) < 0.9, a, rs.randint(0, ids, M))
    a[rs.rand(M) < 0.1] = -1
    b[rs.rand(M) < 0.1] = -1
    return a.astype(np.int32), b.astype(np.int64)


def spread(v):
    return {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def device_phases(a_d, b_d, A, B):
    lib, dev = H.lib(), a_d.device
    M = a_d.numel()
    ws = ops.pairs_workspace(dev, M)
    head = torch.empty(2, dtype=torch.int64, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    st = H.stream_ptr
    ev[0].record()
    H.check(lib.rl_pairs_sort(a_d.data_ptr(), a_d.element_size(), b_d.data_ptr(), b_d.element_size(), M, A, B,
                              head.data_ptr(), ws.data_ptr(), ws.numel(), st()))
    ev[1].record()
    P, flag = head.tolist()
    assert not flag
    pa = torch.empty(P, dtype=torch.int32, device=dev)
    pb = torch.empty(P, dtype=torch.int32, device=dev)
    count = torch.empty(P, dtype=torch.int64, device=dev)
    ev[2].record()
    H.check(lib.rl_pairs_write(M, A, B, P, pa.data_ptr(), pb.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(), st()))
    ev[3].record()
    torch.cuda.synchronize()
    return {"sort": ev[0].elapsed_time(ev[1]), "write": ev[2].elapsed_time(ev[3])}, P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="150000,10000000")
    ap.add_argument("--ids", type=int, default=1000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_pairs measures the MI355X"
    dev = torch.device("cuda", 0)
    A = B = args.ids
    res = {"device": torch.cuda.get_device_name(0), "reps": REPS, "ids": args.ids, "key_bits": IM.key_bits(A, B), "rows": []}
    for M in (int(s) for s in args.sizes.split(",") if s):
        a, b = scene(M, args.ids)
        with torch.cuda.device(dev), torch.no_grad():
            a_d, b_d = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
            runs = [device_phases(a_d, b_d, A, B) for _ in range(WARM + REPS)]
            whole = []
            for _ in range(WARM + REPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = ops.pair_counts(a_d, b_d, A, B)
                torch.cuda.synchronize()
                whole.append((time.perf_counter() - t0) * 1e3)
            del a_d, b_d, out
            torch.cuda.empty_cache()
        timed = [t[0] for t in runs[WARM:]]
        calls = []
        for _ in range(1 + 3):
            t0 = time.perf_counter()
            got = IM.pair_counts(a, b, A, B, device=dev)
            calls.append((time.perf_counter() - t0) * 1e3)
        twins = []
        for _ in range(3):
            t0 = time.perf_counter()
            ref = IM.pair_counts_host(a, b, A, B)
            twins.append((time.perf_counter() - t0) * 1e3)
        row = {"M": M, "pairs": runs[-1][1], "passes": (IM.key_bits(A, B) + 7) // 8}
        for ph in ("sort", "write"):
            row[ph + "_ms"] = spread([t[ph] for t in timed])
        row["device_ms"] = spread([sum(t.values()) for t in timed])
        row["ops_ms"] = spread(whole[WARM:])
        row["call_ms"] = spread(calls[1:])
        row["twin_ms"] = spread(twins)
        row["equals_twin"] = all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(got, ref))
        res["rows"].append(row)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
