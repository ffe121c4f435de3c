#!/usr/bin/env python3
"""Training crops over whole scenes (Model.train_scenes, rl_scenes_* in csrc/scene.hip) on one MI355X.  Prints one JSON line.
Not part of bench.py.  usage: python tools/scene_train_bench.py [--no-train]

  crops      per scene set (16 scenes of 10^6 points, 4 scenes of 10^7; uniform points in 40 x 40 x 4 m boxes), n = 40960:
             crop_us = one rl_scenes_crop with B = 1, batch8_us = one call with B = 8 (device events around 32 calls after a
             warm-up), and the algorithmic bytes of one crop of the picked scene
  train      clouds/s of Model.train_scenes against Model.train on pre-cut 40960-point clouds, both with the device loader in
             rng="device", default augmentation, batch 8, a config-S-shaped network (13 classes, K = 16, layers
             [16, 64, 128, 256, 512]); one timed epoch of 40 steps after a warm-up epoch, timed between the Trainer's per-epoch
             callbacks, so each includes that epoch's validation (one batch x 10 passes)"""
import json
import logging
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "3d_recognizer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from randlanet import _ops as ops  # noqa: E402
from randlanet.utils import scene  # noqa: E402

N, B, C = 40960, 8, 13
LAYERS = [16, 64, 128, 256, 512]
STEPS = 40


def crop_bytes(M: int, n: int) -> int:
    """One crop of a scene of M points: x y z read + d2 keys written (12 + 4 B), keys read by two radix passes, the count pass
    and the write pass (4 x 4 B), possibilities read by the write pass for the key refresh (4 B); the crop's rows (8 B) and its
    possibilities written (4 B)."""
    return (12 + 4 + 16 + 4) * M + n * 12


def scene_set(S: int, M: int, seed: int):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(S):
        xyz = (rs.rand(M, 3) * np.array([40.0, 40.0, 4.0])).astype(np.float32)
        out.append((xyz, np.zeros((M, 0), np.float32), (xyz[:, 2] > 2.0).astype(np.int64) * 3 % C))
    return out


def events_us(fn, reps: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def crops(dev, S: int, M: int) -> dict:
    sizes = [M] * S
    xyz = np.concatenate([x for x, _, _ in scene_set(S, M, S)])
    with torch.cuda.device(dev):
        xyz_d = torch.from_numpy(xyz).to(dev)
        poss = torch.from_numpy(scene.initial_possibility(xyz.shape[0], 0)).to(dev)
        ws = ops.scenes_workspace(dev, S, M, N)
        ops.scenes_init(torch.from_numpy(scene.scene_offsets(sizes)).to(dev), poss, ws, M)
        idx = torch.empty((B, N), dtype=torch.int64, device=dev)
        sc = torch.empty(B, dtype=torch.int64, device=dev)
        one = lambda: ops.scenes_crop(xyz_d, poss, N, idx[:1], sc[:1], ws, S, M)
        eight = lambda: ops.scenes_crop(xyz_d, poss, N, idx, sc, ws, S, M)
        for _ in range(8):
            eight()
        torch.cuda.synchronize()
        crop_us = events_us(one, 32)
        batch_us = events_us(eight, 32)
        hit = len(set(sc.cpu().tolist()))
    del xyz_d, poss, ws
    torch.cuda.empty_cache()
    nb = crop_bytes(M, N)
    return {"scenes": S, "M": M, "crop_us": round(crop_us, 1), "batch8_us": round(batch_us, 1), "crop_bytes": nb,
            "crop_GBps": round(nb / (crop_us * 1e-6) / 1e9, 1), "scenes_in_last_batch": hit}


def train_rate(dev, what: str, data) -> dict:
    from randlanet import AugmentationSettings, Model, RandLANetSettings, TrainingSettings
    torch.manual_seed(0)
    np.random.seed(0)
    model = Model(RandLANetSettings(n_classes=C, n_points=N, n_neighbors=16, layer_sizes=LAYERS))
    stamps = []
    cb = [lambda e, m: (torch.cuda.synchronize(dev), stamps.append(time.perf_counter()))]
    settings = TrainingSettings(epochs=2, batch_size=B, early_stopping=False)
    names = [f"c{i}" for i in range(C)]
    if what == "precut":
        model.train(data[0], data[1], settings, AugmentationSettings(), class_names=names, callbacks=cb)
    else:
        model.train_scenes(data[0], data[1], settings, AugmentationSettings(), crops_per_epoch=STEPS * B,
                           validation_crops=B, center_noise=0.1, class_names=names, callbacks=cb)
    dt = stamps[1] - stamps[0]
    del model
    torch.cuda.empty_cache()
    return {"clouds_per_s": round(STEPS * B / dt, 1), "ms_per_step": round(1e3 * dt / STEPS, 3)}


def main():
    assert torch.cuda.is_available(), "scene_train_bench measures the MI355X"
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    logging.getLogger("trainer").setLevel(logging.WARNING)
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "n": N, "B": B, "crops": [crops(dev, 16, 10 ** 6), crops(dev, 4, 10 ** 7)]}
    if "--no-train" not in sys.argv:
        os.environ["RL_PIPELINE_RNG"] = "device"
        rs = np.random.RandomState(1)
        precut = []
        for _ in range(STEPS * B):
            xyz = (rs.rand(N, 3) * np.array([4.0, 4.0, 4.0])).astype(np.float32)
            precut.append((xyz, np.zeros((N, 0), np.float32), (xyz[:, 2] > 2.0).astype(np.int64)))
        res["train"] = {"precut": train_rate(dev, "precut", (precut, precut[:B]))}
        del precut
        for S, M in ((16, 10 ** 6), (4, 10 ** 7)):
            res["train"][f"scenes_{S}x{M}"] = train_rate(dev, "scenes", (scene_set(S, M, 7), scene_set(1, M, 8)))
        base = res["train"]["precut"]["clouds_per_s"]
        for k, v in res["train"].items():
            v["vs_precut"] = round(v["clouds_per_s"] / base, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
