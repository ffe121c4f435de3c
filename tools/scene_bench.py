#!/usr/bin/env python3
"""Voted-crop scene inference (Model.predict_scene, csrc/scene.hip) on one MI355X: n = 40960 points per crop, B = 8 crops
per pass, scenes of M = 10^6 and 10^7 points (a 40 x 40 x 4 m box of uniform points), a config-S-shaped network
(13 classes, K = 16, layers [16, 64, 128, 256, 512]).  Per M it reports
  crop_us        one rl_scene_crop (pick + select + gather + possibility update), device events around 64 crops
  accumulate_us  one rl_scene_accumulate (softmax + blend of a crop's 13 x 40960 logits)
  pass_ms        one pass as predict_scene runs it: 8 crops, the captured eval forward, 8 blends, the min-count read-back
  crops_per_s    8 / pass_ms, the crop rate of the whole pipeline
  scene_s        a whole predict_scene(votes=1) call (host copy-in, passes until covered, copy-out, normalisation), passes
and the algorithmic bytes of one crop.  Prints one JSON line.  Not part of bench.py.  usage: python tools/scene_bench.py"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "3d_recognizer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from randlanet import Model, RandLANetSettings  # noqa: E402
from randlanet import _ops as ops  # noqa: E402
from randlanet.utils import scene  # noqa: E402

N, B, C = 40960, 8, 13


def crop_bytes(M: int, n: int, dim: int) -> int:
    """Bytes one crop must move: possibility read (pick), x y z read + d2 keys written (select pass 1), keys read by the two
    radix passes, the count pass and the write pass, the crop's rows / indices written, its possibilities read and
    written.  The row reads of a (M, dim) cloud fetch whole rows: 4 * dim bytes per point."""
    return 4 * M + (4 * dim + 4) * M + 4 * 4 * M + n * (4 * dim + 4 * dim + 4 + 8)


def events_ms(fn, reps: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    assert torch.cuda.is_available(), "scene_bench measures the MI355X"
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = Model(RandLANetSettings(n_classes=C, n_points=N, n_neighbors=16, layer_sizes=[16, 64, 128, 256, 512]))
    res = {"device": torch.cuda.get_device_name(0), "n": N, "B": B, "classes": C, "rows": []}
    for M in (10 ** 6, 10 ** 7):
        rs = np.random.RandomState(M % 9973)
        xyz = (rs.rand(M, 3) * np.array([40.0, 40.0, 4.0])).astype(np.float32)
        with torch.cuda.device(dev), torch.no_grad():
            step = model.module.infer_step(B, N)
            cloud = torch.from_numpy(xyz).to(dev)
            poss = torch.from_numpy(scene.initial_possibility(M, 0)).to(dev)
            prob = torch.zeros((M, C), dtype=torch.float32, device=dev)
            count = torch.zeros(M, dtype=torch.int32, device=dev)
            idx = torch.empty((B, N), dtype=torch.int32, device=dev)
            ws = ops.scene_workspace(dev, M, N)
            low = torch.empty(1, dtype=torch.int32, device=dev)
            k = [0]

            def one_crop():
                ops.scene_crop(cloud, poss, N, step.inp[k[0] % B], idx[k[0] % B], ws)
                k[0] += 1

            def one_acc():
                ops.scene_accumulate(step.logits[0], idx[0], 0.05, 0.95, prob, count)

            def one_pass():
                for b in range(B):
                    ops.scene_crop(cloud, poss, N, step.inp[b], idx[b], ws)
                logits = step.step(np.random.permutation(N))
                for b in range(B):
                    ops.scene_accumulate(logits[b], idx[b], 0.05, 0.95, prob, count)
                ops.scene_min_count(count, low, ws)
                int(low.item())

            for _ in range(16):
                one_crop()
            one_pass()
            one_acc()
            torch.cuda.synchronize()
            crop_ms = events_ms(one_crop, 64)
            acc_ms = events_ms(one_acc, 64)
            t0 = time.perf_counter()
            for _ in range(10):
                one_pass()
            pass_ms = (time.perf_counter() - t0) / 10 * 1e3
            del prob, count, poss, ws
        model.predict_scene(xyz[: 200000], batch_size=B)          # warm the whole call path once
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, counts = model.predict_scene(xyz, batch_size=B, return_counts=True)
        scene_s = time.perf_counter() - t0
        nb = crop_bytes(M, N, 3)
        res["rows"].append({
            "M": M, "crop_us": round(crop_ms * 1e3, 1), "crop_bytes": nb,
            "crop_GBps": round(nb / (crop_ms * 1e-3) / 1e9, 1),
            "accumulate_us": round(acc_ms * 1e3, 1), "pass_ms": round(pass_ms, 3),
            "crops_per_s": round(B / (pass_ms * 1e-3), 1),
            "scene_s": round(scene_s, 3), "passes": int(counts.sum()) // (B * N), "min_votes": int(counts.min()),
        })
    print(json.dumps(res))


if __name__ == "__main__":
    main()
