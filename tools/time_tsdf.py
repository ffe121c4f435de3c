#!/usr/bin/env python3
"""TSDF fusion (randlanet/utils/tsdf.py, csrc/tsdf.hip) on one MI355X.  The scene: a tilted, bumpy surface around 0.35 m with
1 mm of noise and a twentieth of holes in an H x W frame (the reference camera's 1024 x 768), fused into a cube of n^3 voxels
and 0.4 m edge on the optical axis, trunc = 4 voxels; a second frame with new noise alternates with the first.
  integrate_us        device events around CALLS consecutive rl_tsdf_integrate calls on frames already in HBM, divided by CALLS:
                      microseconds per call, median [min, max] over REPS windows after warm-up.  One launch
  count_us/points_us  the same for rl_tsdf_count (two launches) and rl_tsdf_points (one launch) on the fused volume, min_weight 1
  copy_us             the same for a plain device copy of 8 bytes per voxel (torch's copy_: 8 bytes read and 8 written per voxel,
                      what integrate moves when every voxel changes), the yardstick for "bandwidth bound", in the same run
  *_gbs               the bytes the algorithm needs over the median: integrate 8 per voxel in, 8 out per voxel of a stored run,
                      2 per pixel; count and points 8 per voxel in (the neighbours come from lines already read), points 20 out
                      per point; the copy 16 per voxel
  extract_ms          the public TsdfVolume.extract: count, the read-back of M, the allocation, points
  twin_*_ms           integrate_host and extract_host on the same volume (numpy, this machine's CPUs)
  add_ms              one DepthFusion.add with tracking on a GPU-placed model: depth_points at track_stride, extract, ICP
                      (point to plane, normals of the surface estimated per call), integrate; the camera does not move
Prints one JSON line.  Not part of bench.py, not run by any test.
usage: python tools/time_tsdf.py [--height 768] [--width 1024] [--sizes 128 256] [--no-fusion]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "3d_recognizer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from randlanet import _ops as ops  # noqa: E402
from randlanet.utils import depth as D  # noqa: E402
from randlanet.utils import registration as R  # noqa: E402
from randlanet.utils import tsdf as T  # noqa: E402

REPS, WARM, CALLS = 9, 3, 20
SCALE = 0.00025
EDGE, CENTRE = 0.4, 0.35


def frames(H: int, W: int):
    rs = np.random.RandomState(H * 7 + W)
    v, u = np.mgrid[0:H, 0:W]
    z = CENTRE + 0.12 * (0.6 * u / W + 0.4 * v / H - 0.5) + 0.02 * np.sin(u / 37.0) * np.cos(v / 29.0)
    out = []
    for _ in range(2):
        d = np.round((z + 0.001 * rs.randn(H, W)) / SCALE).astype(np.uint16)
        d[rs.uniform(size=(H, W)) < 0.05] = 0
        out.append(d)
    return out


def spread(v, digits=1):
    return {"median": round(float(np.median(v)), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def windows(call, calls=CALLS):
    """Microseconds per call of `call(i)`: REPS windows of `calls` calls between two events, after WARM windows."""
    us = []
    for _ in range(WARM + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(calls):
            call(i)
        e1.record()
        torch.cuda.synchronize()
        us.append(1000.0 * e0.elapsed_time(e1) / calls)
    return us[WARM:]


def wall(fn, reps=5, warm=1):
    ms = []
    for _ in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1000.0 * (time.perf_counter() - t0))
    return ms[warm:]


def gbs(nbytes, us):
    return round(nbytes / (us["median"] * 1e-6) / 1e9, 1)


def volume(n: int, device):
    voxel = EDGE / n
    return T.TsdfVolume((-EDGE / 2, -EDGE / 2, CENTRE - EDGE / 2), voxel, (n, n, n), device=device)


def one_size(n, pair, pair_d, cam, z_lo, z_hi, dev):
    V = n ** 3
    H, W = pair[0].shape
    w2c = T.world_to_camera(np.eye(4))
    res = {"n": n, "voxels": V}
    with torch.cuda.device(dev), torch.no_grad():
        vol = volume(n, dev)
        # one frame against the twin: faster and different is not faster
        host = volume(n, "cpu")
        t0 = time.perf_counter()
        host.integrate(pair[0], cam)
        res["twin_integrate_ms"] = round(1000.0 * (time.perf_counter() - t0), 1)
        vol.integrate(pair_d[0], cam)
        same = np.array_equal(vol.tsdf.cpu().numpy().view(np.uint32), host.tsdf.view(np.uint32)) and \
            np.array_equal(vol.weight.cpu().numpy(), host.weight)
        t0 = time.perf_counter()
        want = host.extract(1)
        res["twin_extract_ms"] = round(1000.0 * (time.perf_counter() - t0), 1)
        got = vol.extract(1)
        same = same and np.array_equal(got.edge.cpu().numpy(), want.edge) and \
            np.array_equal(got.xyz.cpu().numpy().view(np.uint32), want.xyz.view(np.uint32))
        res["equals_twin"] = bool(same)
        runs = host.weight.reshape(-1, 4).any(axis=1)                # (n is a multiple of 4: a run does not straddle rows)
        res["updated"] = round(float((host.weight > 0).mean()), 3)
        res["stored_runs"] = round(float(runs.mean()), 3)

        def integrate(i):
            ops.tsdf_integrate(vol.tsdf, vol.weight, vol.origin, vol.voxel, vol.trunc, vol.max_weight, pair_d[i & 1], cam, z_lo,
                               z_hi, w2c)

        res["integrate_us"] = spread(windows(integrate))
        res["integrate_gbs"] = gbs(8 * V + 32 * int(runs.sum()) + 2 * H * W, res["integrate_us"])
        count = torch.empty(1, dtype=torch.int64, device=dev)
        ws = ops.tsdf_workspace(dev, V)
        head = ops._tsdf_volume(vol.tsdf, vol.weight, vol.origin, vol.voxel)
        lib = ops.H.lib()
        res["count_us"] = spread(windows(lambda i: ops.H.check(lib.rl_tsdf_count(*head, 1, count.data_ptr(), ws.data_ptr(), ws.numel(),
                                                                                 ops._st()))))
        M = int(count.item())
        res["points"] = M
        xyz = torch.empty((M, 3), dtype=torch.float32, device=dev)
        edge = torch.empty(M, dtype=torch.int64, device=dev)
        res["points_us"] = spread(windows(lambda i: ops.H.check(lib.rl_tsdf_points(*head, 1, M, xyz.data_ptr(), edge.data_ptr(), M,
                                                                                   ws.data_ptr(), ws.numel(), ops._st()))))
        res["count_gbs"] = gbs(8 * V, res["count_us"])
        res["points_gbs"] = gbs(8 * V + 20 * M, res["points_us"])
        src = torch.empty(2 * V, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        res["copy_us"] = spread(windows(lambda i: dst.copy_(src)))
        res["copy_gbs"] = gbs(16 * V, res["copy_us"])
        res["extract_ms"] = spread(wall(lambda: vol.extract(1)), 3)
    return res


def fusion_times(n, pair, cam, dev, stride):
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    model = Model(RandLANetSettings(n_classes=4, n_points=16384, n_neighbors=16, layer_sizes=[16, 32, 64, 128]), use_gpu=True)
    fusion = T.DepthFusion(model, cam, volume(n, dev), icp=R.IcpSettings(max_distance=0.01), track_stride=stride)
    first = fusion.add(pair[0])
    status = []

    def add():
        status.append(fusion.add(pair[len(status) & 1]).status)

    ms = wall(add, reps=7, warm=2)
    surf = fusion.surface()
    return {"n": n, "track_stride": stride, "source_points": int(D.deproject_host(pair[0], cam, stride=stride).pixel.shape[0]),
            "surface_points": int(surf.xyz.shape[0]), "add_ms": spread(ms, 2), "status": sorted(set(status)), "first": first.status}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--track-stride", type=int, default=4)
    ap.add_argument("--no-fusion", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_tsdf measures the MI355X"
    dev = torch.device("cuda", 0)
    H, W = args.height, args.width
    cam = D.DepthCamera(W, H, 730.5, 731.25, W / 2 - 0.2, H / 2 + 0.3, SCALE)
    pair = frames(H, W)
    z_lo, z_hi, _ = D.check_inputs(pair[0], cam, (0.05, 0.6), 1)
    res = {"device": torch.cuda.get_device_name(0), "H": H, "W": W, "reps": REPS, "calls_per_window": CALLS, "sizes": []}
    with torch.cuda.device(dev):
        pair_d = [torch.from_numpy(f).to(dev) for f in pair]
    for n in args.sizes:
        assert n % 4 == 0
        res["sizes"].append(one_size(n, pair, pair_d, cam, z_lo, z_hi, dev))
    if not args.no_fusion:
        res["fusion"] = fusion_times(args.sizes[0], pair, cam, dev, args.track_stride)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
