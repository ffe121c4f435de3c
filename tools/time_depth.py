#!/usr/bin/env python3
"""Depth frames to points (randlanet/utils/depth.py, csrc/depth.hip) on one MI355X.  The frame: H x W (the reference camera's
1024 x 768) raw z16 values of a tilted surface with noise between 0.1 m and 0.9 m and a tenth of holes, so that about half the
pixels lie inside z_range = (0.05, 0.6); a second frame of the same scene with new noise feeds the temporal filter.
  points_us / filtered_us   device events around CALLS consecutive rl_depth_points calls on a frame already in HBM, without and
                            with the temporal filter (its state resident, the two frames alternating), divided by CALLS:
                            microseconds per call, median [min, max] over REPS windows after warm-up.  Three launches each
  filter_us                 the same for the filter alone (TemporalFilter.process's entry: one launch)
  call_ms                   the public depth_points(device="cuda") on a numpy frame: upload, kernels, the read-back of M
  twin_ms / twin_filtered_ms  deproject_host, and the host filter followed by it, on the same frame (numpy, this machine's CPUs)
  predict_depth_ms          Model.predict_depth of the frame on a GPU-placed model (a small network, n_points = 16384), against
  host_predict_ms           deproject_host + Model.predict on the same model; the two alternate, wall-clock after warm-up
Prints one JSON line.  Not part of bench.py, not run by any test.
usage: python tools/time_depth.py [--height 768] [--width 1024] [--stride 1] [--no-model]"""
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

REPS, WARM, CALLS = 9, 3, 50
SCALE = 0.00025


def frames(H: int, W: int):
    rs = np.random.RandomState(H * 7 + W)
    v, u = np.mgrid[0:H, 0:W]
    z = 0.1 + 0.8 * (0.6 * u / W + 0.4 * v / H)
    out = []
    for _ in range(2):
        d = np.round((z + 0.002 * rs.randn(H, W)) / SCALE).astype(np.uint16)
        d[rs.uniform(size=(H, W)) < 0.1] = 0
        out.append(d)
    return out


def spread(v, digits=1):
    return {"median": round(float(np.median(v)), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def windows(call):
    """Microseconds per call of `call(i)`: REPS windows of CALLS calls between two events, after WARM windows."""
    us = []
    for _ in range(WARM + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(CALLS):
            call(i)
        e1.record()
        torch.cuda.synchronize()
        us.append(1000.0 * e0.elapsed_time(e1) / CALLS)
    return us[WARM:]


def wall(fn, reps=7, warm=2):
    ms = []
    for _ in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1000.0 * (time.perf_counter() - t0))
    return ms[warm:]


def same(a: D.DepthCloud, b: D.DepthCloud) -> bool:
    ax, ap = (t.cpu().numpy() if torch.is_tensor(t) else t for t in a)
    return bool(np.array_equal(ap, b.pixel) and np.array_equal(ax.view(np.uint32), b.xyz.view(np.uint32)))


def model_times(frame, cam, stride):
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    model = Model(RandLANetSettings(n_classes=4, n_points=16384, n_neighbors=16, layer_sizes=[16, 32, 64, 128]), use_gpu=True)

    def on_device():
        np.random.seed(0)
        return model.predict_depth(frame, cam, stride=stride)

    def on_host():
        np.random.seed(0)
        return model.predict(D.deproject_host(frame, cam, stride=stride).xyz)

    for _ in range(2):
        a, b = on_device(), on_host()
    dev_ms, host_ms = [], []
    for _ in range(9):                  # alternating: the two share whatever else the host is doing
        dev_ms += wall(on_device, reps=1, warm=0)
        host_ms += wall(on_host, reps=1, warm=0)
    return {"n_points": 16384, "predict_depth_ms": spread(dev_ms, 2), "host_predict_ms": spread(host_ms, 2),
            "equal": bool(np.array_equal(a.confidences.view(np.uint32), b.view(np.uint32)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_depth measures the MI355X"
    dev = torch.device("cuda", 0)
    H, W, stride = args.height, args.width, args.stride
    cam = D.DepthCamera(W, H, 730.5, 731.25, W / 2 - 0.2, H / 2 + 0.3, SCALE)
    pair = frames(H, W)
    z_lo, z_hi, _ = D.check_inputs(pair[0], cam, (0.05, 0.6), stride)
    filt = D.TemporalFilter()
    res = {"device": torch.cuda.get_device_name(0), "H": H, "W": W, "stride": stride, "reps": REPS, "calls_per_window": CALLS}
    with torch.cuda.device(dev), torch.no_grad():
        pair_d = [torch.from_numpy(f).to(dev) for f in pair]
        P = H * W
        xyz = torch.empty((P, 3), dtype=torch.float32, device=dev)
        pixel = torch.empty(P, dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        out = torch.empty((H, W), dtype=torch.uint16, device=dev)
        state = torch.zeros((H, W), dtype=torch.int16, device=dev).view(torch.uint16)
        ws = ops.depth_workspace(dev, P)
        par = (filt.alpha, filt.one_minus_alpha, filt.delta)
        res["points_us"] = spread(windows(lambda i: ops._depth_call(pair_d[0], None, None, cam, stride, None, z_lo, z_hi, xyz, pixel,
                                                                    count, ws)))
        res["kept"] = int(count.item())
        res["filtered_us"] = spread(windows(lambda i: ops._depth_call(pair_d[i & 1], state, None, cam, stride, par, z_lo, z_hi, xyz,
                                                                      pixel, count, ws)))
        res["filter_us"] = spread(windows(lambda i: ops._depth_call(pair_d[i & 1], state, out, cam, 1, par, z_lo, z_hi, None, None,
                                                                    None, None)))
    res["call_ms"] = spread(wall(lambda: D.depth_points(pair[0], cam, stride=stride, device=dev)), 3)
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        twin = D.deproject_host(pair[0], cam, stride=stride)
        t.append(1000.0 * (time.perf_counter() - t0))
    res["twin_ms"] = spread(t, 2)
    host = D.TemporalFilter()
    host.process(pair[1], device="cpu")
    t = []
    for k in range(5):
        t0 = time.perf_counter()
        D.depth_points(pair[k & 1], cam, host, stride=stride, device="cpu")
        t.append(1000.0 * (time.perf_counter() - t0))
    res["twin_filtered_ms"] = spread(t, 2)
    res["equals_twin"] = same(D.depth_points(pair[0], cam, stride=stride, device=dev), twin)
    if not args.no_model:
        res["model"] = model_times(pair[0], cam, stride)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
