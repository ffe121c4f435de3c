#!/usr/bin/env python3
"""RANSAC plane segmentation (randlanet/utils/planes.py, csrc/planes.hip) on one MI355X.  Clouds: a desk under clutter - 40 %
of the M points on a noisy plane, the rest uniform in a box above it - with M = 150000, 501221 (a 1024 x 768 camera frame
after the range gate) and 10^7, T = 256 and 1024 hypotheses, threshold 0.01.  Per cloud and T:
  hyp_ms / count_ms / split_ms   device events around rl_planes_hypotheses (1 launch), rl_planes_count (3: the T * M tests,
                        the table's column sums, the maximum) and rl_planes_split (3) on coordinates already in HBM; median
                        [min, max] in ms over REPS passes after WARM warm-ups
  tests_per_s           T * M / the median of count_ms, next to valu_bound: what 256 CUs x 4 SIMDs x 2.4 GHz / 4 cycles per
                        wavefront instruction give at the 5.0625 vector instructions per test of pl_count's compiled inner
                        loop (81 per 8 points x 2 hypotheses: 24 v_pk_mul_f32, 24 v_pk_add_f32, 16 v_cmp_le_f32, 8 v_cndmask,
                        8 v_addc_co_u32, 1 loop compare)
  fit_ms                the whole _ops.fit_plane on the device cloud - hypotheses, count, split, moments, refinement, split -
                        with its two read-backs, wall clock
  twin_s                fit_plane_host on the same input (numpy, this machine's CPUs), up to --twin-max points
With --keypoints: one Model.predict_keypoints (a small network, votes = 1) from the 501221-point cloud as a device tensor with
grid=, with and without remove_planes=, wall-clock seconds after one warm-up call each.
Prints one JSON line.  Not part of bench.py, not run by any test.
usage: python tools/time_planes.py [--sizes 150000,501221,10000000] [--iterations 256,1024] [--twin-max 501221] [--keypoints]"""
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
from randlanet.utils import planes as P  # noqa: E402

REPS, WARM = 5, 2
THRESHOLD = 0.01
VALU_PER_TEST = 81 / 16
VALU_BOUND = 256 * 4 * 2.4e9 / 4 * 64 / VALU_PER_TEST        # tests per second


def desk(M: int) -> np.ndarray:
    rs = np.random.RandomState(M % 9973)
    n = int(0.4 * M)
    side = np.sqrt(M / 250000.0)
    plane = np.concatenate([rs.rand(n, 2) * side, 0.003 * rs.randn(n, 1)], axis=1)
    rest = rs.rand(M - n, 3) * (side, side, 0.4) + (0, 0, 0.02)
    return np.ascontiguousarray(np.concatenate([plane, rest])[rs.permutation(M)], dtype=np.float32)


def spread(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def one_pass(xyz_d, tri_d, T):
    """The three entries with an event pair around each; returns (hyp, count, split) in ms and the best count."""
    lib, dev, M = H.lib(), xyz_d.device, xyz_d.shape[0]
    hyp = torch.empty((T, 4), dtype=torch.float32, device=dev)
    flags = torch.empty(4, dtype=torch.int32, device=dev)
    counts = torch.empty(T, dtype=torch.int32, device=dev)
    inlier = torch.empty(M, dtype=torch.uint8, device=dev)
    slot = torch.empty(M, dtype=torch.int32, device=dev)
    kept = torch.empty(M, dtype=torch.int64, device=dev)
    n = torch.empty(1, dtype=torch.int64, device=dev)
    ws = ops.planes_workspace(dev, M, T)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    st = H.stream_ptr()
    e[0].record()
    H.check(lib.rl_planes_hypotheses(xyz_d.data_ptr(), M, tri_d.data_ptr(), T, None, 0.0, hyp.data_ptr(), flags.data_ptr(), st))
    e[1].record()
    H.check(lib.rl_planes_count(xyz_d.data_ptr(), M, hyp.data_ptr(), T, THRESHOLD, counts.data_ptr(), flags[1:].data_ptr(),
                                ws.data_ptr(), ws.numel(), st))
    e[2].record()
    H.check(lib.rl_planes_split(xyz_d.data_ptr(), M, hyp.data_ptr(), flags[1:].data_ptr(), THRESHOLD, inlier.data_ptr(),
                                slot.data_ptr(), kept.data_ptr(), n.data_ptr(), ws.data_ptr(), ws.numel(), st))
    e[3].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]), e[2].elapsed_time(e[3]), int(flags[2].item())


def keypoint_times(xyz_d, cell):
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    model = Model(RandLANetSettings(n_classes=4, n_points=16384, n_neighbors=16, layer_sizes=[16, 32, 64, 128]), use_gpu=True)
    out = {"M": int(xyz_d.shape[0]), "cell": cell}
    for name, kw in (("plain_s", {}), ("remove_planes_s", {"remove_planes": P.PlaneRemoval(THRESHOLD)})):
        t = []
        for _ in range(2):
            np.random.seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = model.predict_keypoints(xyz_d, radius=0.05, grid=cell, votes=1, batch_size=8, return_planes=True, **kw)
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        out[name] = round(t[1], 4)
        out[name.replace("_s", "_plane_points")] = int((res[1][1] >= 0).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="150000,501221,10000000")
    ap.add_argument("--iterations", default="256,1024")
    ap.add_argument("--twin-max", type=int, default=501221)
    ap.add_argument("--keypoints", action="store_true")
    ap.add_argument("--cell", type=float, default=0.01)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_planes measures the MI355X"
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "reps": REPS, "threshold": THRESHOLD,
           "valu_per_test": VALU_PER_TEST, "valu_bound_tests_per_s": VALU_BOUND, "rows": []}
    for M in (int(s) for s in args.sizes.split(",") if s):
        xyz = desk(M)
        for T in (int(s) for s in args.iterations.split(",") if s):
            tri = P.draw_triples(np.random.default_rng(0), M, T)
            with torch.cuda.device(dev), torch.no_grad():
                xyz_d, tri_d = torch.from_numpy(xyz).to(dev), torch.from_numpy(tri).to(dev)
                runs = [one_pass(xyz_d, tri_d, T) for _ in range(WARM + REPS)][WARM:]
                fits = []
                for _ in range(WARM + REPS):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got = ops.fit_plane(xyz_d, tri, THRESHOLD)
                    torch.cuda.synchronize()
                    fits.append(1e3 * (time.perf_counter() - t0))
                del xyz_d
            cols = [[r[j] for r in runs] for j in range(3)]
            rate = T * M / (1e-3 * float(np.median(cols[1])))
            row = {"M": M, "T": T, "workspace_bytes": int(H.lib().rl_planes_workspace_bytes(M, T)), "best_count": runs[0][3],
                   "refined_count": int(got[4]), "hyp_ms": spread(cols[0]), "count_ms": spread(cols[1]),
                   "split_ms": spread(cols[2]), "tests_per_s": float(f"{rate:.4g}"), "of_valu_bound": round(rate / VALU_BOUND, 3),
                   "fit_ms": spread(fits[WARM:])}
            if M <= args.twin_max:
                t0 = time.perf_counter()
                ref = P.fit_plane_host(xyz, THRESHOLD, triples=tri)
                row["twin_s"] = round(time.perf_counter() - t0, 3)
                row["equals_twin"] = bool(np.array_equal(got[0].view(np.uint32), ref.plane.view(np.uint32))
                                          and np.array_equal(got[6].cpu().numpy(), ref.counts)
                                          and np.array_equal(got[1].cpu().numpy(), ref.inlier))
            res["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    if args.keypoints:
        with torch.cuda.device(dev):
            res["predict_keypoints"] = keypoint_times(torch.from_numpy(desk(501221)).to(dev), args.cell)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
