#!/usr/bin/env python3
"""The union step of the clustering (csrc/cluster.hip) on one MI355X under the density rule, and this build against another:
  ms1          rl_cluster_union of this build: what min_samples = 1 launches
  ms4, ms16    rl_cluster_union_dense of this build at min_samples = 4 and 16 (--min-samples): support, union between core
               points, attach, flatten
  baseline     rl_cluster_union of the library given by --baseline-lib (a librandla_hip.so built from another revision, for
               instance the parent commit's): the check that templating the kernels left the plain path where it was
Scene: the uniform one of tools/time_clusters.py (40 x 40 x 4 m, 12 classes in 2 m columns over an ignored floor, r chosen for
about ten neighbours within r) at every size of --sizes.  The entries are timed by device events on data already in HBM, in
ROUNDS rounds that run them one after another - baseline, ms1, ms4, ms16, baseline, .. - after WARM warm-up rounds, so that a
drift of the machine falls on all of them alike; per entry median [min, max] in ms.  ms1's instance ids are compared with the
baseline's, and up to --twin-max points every entry's with the numpy twin's, whose time is taken too.
Prints one JSON line per size, then one with all of them.  Not part of bench.py, not run by any test.
usage: python tools/time_dbscan.py [--sizes 150000,10000000] [--min-samples 4,16] [--baseline-lib PATH] [--twin-max 10000000]"""
import argparse
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "3d_recognizer_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from randlanet import _hip as H  # noqa: E402
from randlanet import _ops as ops  # noqa: E402
from randlanet.utils import cluster as K  # noqa: E402
from time_clusters import spread, uniform_scene  # noqa: E402

ROUNDS, WARM = 11, 2


def other_library(path):
    lib = ctypes.CDLL(path)
    for name in ("rl_cluster_workspace_bytes", "rl_cluster_cells", "rl_cluster_union", "rl_last_error"):
        res, args = H._SIGNATURES[name]
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="150000,10000000")
    ap.add_argument("--min-samples", default="4,16")
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--twin-max", type=int, default=10000000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_dbscan measures the MI355X"
    dev = torch.device("cuda", 0)
    lib = H.lib()
    base = other_library(args.baseline_lib) if args.baseline_lib else None
    dense = [int(s) for s in args.min_samples.split(",") if s]
    assert all(m > 1 for m in dense), "--min-samples: the dense entries, each above 1"
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "rows": []}
    for M in (int(s) for s in args.sizes.split(",") if s):
        xyz, labels, r, _ = uniform_scene(M)
        r32 = float(np.float32(r))
        with torch.cuda.device(dev), torch.no_grad():
            xyz_d, labels_d = (torch.from_numpy(a).to(dev) for a in (xyz, labels))
            ignore_d = torch.zeros(1, dtype=torch.int64, device=dev)
            ws = ops.dense_cluster_workspace(dev, M, False)
            head = torch.empty(4, dtype=torch.int64, device=dev)
            order = (["baseline"] if base is not None else []) + ["ms1"] + [f"ms{m}" for m in dense]
            out = {k: torch.empty(M, dtype=torch.int32, device=dev) for k in order}
            st = H.stream_ptr
            H.check(lib.rl_cluster_cells(xyz_d.data_ptr(), M, r32, head.data_ptr(), ws.data_ptr(), ws.numel(), st()))
            dims = head[:3].tolist()
            K.check_dims(dims)
            bits = K.key_bits(dims)
            if base is not None:        # (its own copy of the grid state: the same bytes, written by its own kernels)
                assert base.rl_cluster_workspace_bytes(M) == lib.rl_cluster_workspace_bytes(M)
                assert base.rl_cluster_cells(xyz_d.data_ptr(), M, r32, head.data_ptr(), ws.data_ptr(), ws.numel(), st()) == 0
                assert head[:3].tolist() == dims

            def union(which):
                common = (xyz_d.data_ptr(), labels_d.data_ptr(), M, r32, ignore_d.data_ptr(), 1, bits, 1)
                tail = (out[which].data_ptr(), head[3:].data_ptr(), ws.data_ptr(), ws.numel(), st())
                if which in ("baseline", "ms1"):
                    return (lib if which == "ms1" else base).rl_cluster_union(*common, *tail)
                return lib.rl_cluster_union_dense(*common, None, None, 0.0, 0.0, int(which[2:]), *tail)

            times = {k: [] for k in order}
            count = {}
            for rnd in range(WARM + ROUNDS):
                for which in order:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    rc = union(which)
                    e1.record()
                    torch.cuda.synchronize()
                    assert rc == 0, (which, rc)
                    count[which] = int(head[3].item())
                    if rnd >= WARM:
                        times[which].append(e0.elapsed_time(e1))
            ids = {k: v.cpu().numpy() for k, v in out.items()}
            del xyz_d, labels_d, ws, out
            torch.cuda.empty_cache()
        row = {"M": M, "radius": r, "dims": dims, "instances": count,
               "noise": {k: int((v < 0).sum() - (labels == 0).sum()) for k, v in ids.items()}}
        for k in order:
            row[k + "_union_ms"] = spread(times[k])
        if base is not None:
            row["ms1_equals_baseline"] = bool(np.array_equal(ids["ms1"], ids["baseline"]))
        if M <= args.twin_max:
            for k in order[1 if base is not None else 0:]:
                t0 = time.perf_counter()
                ref = K.euclidean_clusters_host(xyz, labels, radius=r, min_samples=int(k[2:]))
                row[f"twin_{k}_s"] = round(time.perf_counter() - t0, 3)
                row[f"{k}_equals_twin"] = bool(np.array_equal(ids[k], ref.instance))
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
