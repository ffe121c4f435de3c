#!/usr/bin/env python3
"""Global registration (randlanet/utils/registration.py: global_registration; csrc/fpfh.hip, csrc/match.hip, csrc/global.hip)
on one MI355X.  Clouds: a room corner with a dome, a box and a tilted slab, M samples of it as the target and the same
samples, permuted, with noise of a fifth of the point spacing and moved by 120 degrees and a shift, as the source; M = 5000,
20000 (what a camera frame is after a 1 to 2 cm voxel) and 100000; max_distance = three point spacings, k = 30, normals = 16,
T = 65536.  Per size, device events on clouds already in HBM, median
[min, max] in ms over REPS passes after WARM warm-ups:
  normals_ms        _ops.estimate_normals of the source (k = 16, with a viewpoint)
  descriptor_ms     _ops.fpfh of the source: rl_knn_f32 for k + 1 rows, rl_fpfh_spfh, rl_fpfh_fpfh
  match_ms          rl_match_u8, Ms * Mt * 9 packed dot products; match_gdot_s = that many per second, and match_fraction =
                    its share of the VALU rate at 4 cycles per wavefront instruction: 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz
  hypotheses_ms     rl_global_hypotheses plus rl_global_count (T * C tests); count_gtest_s = tests per second
  sums_ms           rl_global_sums
  global_ms         the whole _ops-level global registration of device clouds, wall clock, read-backs and Kabsch included
  twin_s            global_registration_host on the same input (numpy, this machine's CPUs), up to --twin-max points;
                    equals_twin: every field bit for bit
Prints one JSON line.  Not part of bench.py, not run by any test.
usage: python tools/time_global_registration.py [--sizes 5000,20000,100000] [--twin-max 20000]"""
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
from randlanet.utils import features as F  # noqa: E402
from randlanet.utils import registration as R  # noqa: E402

REPS, WARM = 5, 2
T = 65536
VALU_DOT_RATE = 256 * 4 * 16 * 2.4e9
VIEWPOINT = np.array([1.2, 1.1, 1.5])


def scene(M: int, seed: int) -> np.ndarray:
    rs = np.random.RandomState(seed)
    n = M // 8
    u = rs.uniform(0, 1, (2 * n, 2))
    floor = np.concatenate([u, (0.02 * np.sin(6 * u[:, 0]) * np.cos(5 * u[:, 1]))[:, None]], axis=1)
    v = rs.uniform(0, 1, (n, 2))
    wall_x = np.stack((np.zeros(n), v[:, 0], v[:, 1]), axis=1)
    v = rs.uniform(0, 1, (n, 2))
    wall_y = np.stack((v[:, 0], np.zeros(n), v[:, 1]), axis=1)
    d = rs.normal(size=(n, 3))
    d[:, 2] = np.abs(d[:, 2])
    dome = np.array([0.55, 0.5, 0.0]) + 0.2 * d / np.linalg.norm(d, axis=1, keepdims=True)
    u = rs.uniform(0, 1, (n, 2))
    top = np.stack((0.1 + 0.25 * u[:, 0], 0.55 + 0.3 * u[:, 1], np.full(n, 0.18)), axis=1)
    u = rs.uniform(0, 1, (M - 6 * n, 2))
    slab = np.stack((0.55 + 0.35 * u[:, 0], 0.5 + 0.4 * u[:, 1], 0.3 + 0.4 * u[:, 0] + 0.15 * u[:, 1]), axis=1)
    return np.concatenate([floor, wall_x, wall_y, dome, top, slab])[rs.permutation(M)]


def motion(degrees, shift):
    a, t = np.array([1.0, 2.0, 2.0]) / 3.0, np.radians(degrees)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K), shift
    return M


def spread(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def events(fn):
    """Device ms of fn() between two events: REPS values after WARM warm-ups."""
    ms = []
    for _ in range(WARM + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms[WARM:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5000,20000,100000")
    ap.add_argument("--twin-max", type=int, default=20000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_global_registration measures the MI355X"
    dev = torch.device("cuda", 0)
    lib = H.lib()
    res = {"device": torch.cuda.get_device_name(0), "reps": REPS, "hypotheses": T, "rows": []}
    for M in (int(s) for s in args.sizes.split(",") if s):
        spacing = float(np.sqrt(4.0 / M))
        Mo = motion(120.0, (0.4, -0.3, 0.2))
        tgt_h = scene(M, 1).astype(np.float32)
        rs = np.random.RandomState(M)
        noisy = tgt_h[rs.permutation(M)].astype(np.float64) + rs.normal(scale=0.2 * spacing, size=(M, 3))
        src_h = ((noisy - Mo[:3, 3]) @ Mo[:3, :3]).astype(np.float32)
        vp_s = (VIEWPOINT - Mo[:3, 3]) @ Mo[:3, :3]
        kw = dict(max_distance=3 * spacing, k=30, normals=16, iterations=T, seed=0, source_viewpoint=vp_s, target_viewpoint=VIEWPOINT)
        chk = R.check_global_parameters(kw["max_distance"], 30, 16, T, 0, 0.9)
        tri = R.check_global_triples(None, M, chk)
        with torch.cuda.device(dev), torch.no_grad():
            src, tgt = torch.from_numpy(src_h).to(dev), torch.from_numpy(tgt_h).to(dev)
            vps = np.asarray(vp_s, np.float64).astype(np.float32)
            nrm_ms = events(lambda: ops.estimate_normals(src, 16, vps))
            ns, nt = ops.estimate_normals(src, 16, vps)[0], ops.estimate_normals(tgt, 16, VIEWPOINT.astype(np.float32))[0]
            desc_ms = events(lambda: ops.fpfh(src, ns, 30))
            cs, ct = ops.fpfh(src, ns, 30)[1], ops.fpfh(tgt, nt, 30)[1]
            match_ms = events(lambda: ops.match_features(cs, ct))
            corr = ops.match_features(cs, ct)[0]
            tr = torch.from_numpy(tri).to(dev)
            hyp = torch.empty((T, 12), dtype=torch.float32, device=dev)
            head = torch.empty(T + 1, dtype=torch.int32, device=dev)
            inl = torch.empty(M, dtype=torch.uint8, device=dev)
            out = torch.empty(16, dtype=torch.float64, device=dev)
            ws = ops.global_workspace(dev, M, T)
            st = H.stream_ptr()

            def hyp_count():
                H.check(lib.rl_global_hypotheses(src.data_ptr(), M, tgt.data_ptr(), M, corr.data_ptr(), tr.data_ptr(), T, float(chk.s2),
                                                 hyp.data_ptr(), head.data_ptr(), ws.data_ptr(), ws.numel(), st))
                H.check(lib.rl_global_count(src.data_ptr(), M, tgt.data_ptr(), M, corr.data_ptr(), hyp.data_ptr(), T, float(chk.g2),
                                            head[1:].data_ptr(), ws.data_ptr(), ws.numel(), st))

            hyp_ms = events(hyp_count)
            rt = ops._icp_rt(Mo)
            sums_ms = events(lambda: H.check(lib.rl_global_sums(src.data_ptr(), M, tgt.data_ptr(), M, corr.data_ptr(), rt, float(chk.g2),
                                                                inl.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), st)))
            s = F.check_inputs(src_h, 30, None, 16, vp_s)
            t = F.check_inputs(tgt_h, 30, None, 16, VIEWPOINT)
            walls = []
            for _ in range(WARM + REPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = R.global_registration_device((src,) + s[1:], (tgt,) + t[1:], tri, chk, dev)
                torch.cuda.synchronize()
                walls.append(1e3 * (time.perf_counter() - t0))
            dR = got.transformation[:3, :3] @ Mo[:3, :3].T
            med_match, med_hyp = float(np.median(match_ms)), float(np.median(hyp_ms))
            row = {"M": M, "normals_ms": spread(nrm_ms), "descriptor_ms": spread(desc_ms), "match_ms": spread(match_ms),
                   "match_gdot_s": round(9.0 * M * M / med_match / 1e6, 1),
                   "match_fraction": round(9.0 * M * M / (med_match * 1e-3) / VALU_DOT_RATE, 3),
                   "hypotheses_ms": spread(hyp_ms), "count_gtest_s": round(float(T) * M / med_hyp / 1e6, 1), "sums_ms": spread(sums_ms),
                   "global_ms": spread(walls[WARM:]), "status": got.status, "count": got.count,
                   "valid_hypotheses": int((~np.isnan(got.hypotheses[:, 0])).sum()),
                   "rotation_error_deg": round(float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))), 3)}
            if M <= args.twin_max:
                t0 = time.perf_counter()
                ref = R.global_registration_host(src_h, tgt_h, **kw)
                row["twin_s"] = round(time.perf_counter() - t0, 3)
                row["equals_twin"] = bool(np.array_equal(got.transformation, ref.transformation) and got.count == ref.count
                                          and np.array_equal(got.counts, ref.counts) and np.array_equal(got.sums, ref.sums)
                                          and np.array_equal(got.hypotheses, ref.hypotheses, equal_nan=True)
                                          and np.array_equal(got.correspondence.cpu().numpy(), ref.correspondence)
                                          and np.array_equal(got.inlier.cpu().numpy(), ref.inlier))
            res["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del src, tgt
    print(json.dumps(res))


if __name__ == "__main__":
    main()
