#!/usr/bin/env python3
"""Whole-set scene evaluation on one MI355X, scene by scene against all scenes together (Model.evaluate_scenes with
together=False - the loop over predict_scene's passes - and together=True - Model.predict_scenes' shared passes,
rl_scenes_vote_*): 64 scenes of uniform points at n = 40960 points per crop, B = 8 crops per pass, votes = 1,
pad_small_scenes=True, a config-S-shaped network (13 classes, K = 16, layers [16, 64, 128, 256, 512]).  Two sets:
  small   every scene below n (10k .. 40k points): a scene needs one crop, the loop pays one forward of 8 per scene
  mixed   10k .. 120k points: one to a few crops per scene
Per set and path it reports the forwards run (passes) and the seconds of the whole evaluate_scenes call (host copy-in,
passes, confusion), the better of two runs after one warm-up call, and checks that both paths count every labelled point.
Prints one JSON line.  Not part of bench.py.  usage: python tools/scenes_vote_bench.py"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "3d_recognizer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from randlanet import Model, RandLANetSettings  # noqa: E402

N, B, C, S = 40960, 8, 13, 64


def make_set(lo: int, hi: int, seed: int):
    """S scenes of lo .. hi uniform points at the density of tools/scene_bench.py's box, 4 m high."""
    rs = np.random.RandomState(seed)
    scenes = []
    for M in rs.randint(lo, hi + 1, S):
        side = float(np.sqrt(M / 625.0))
        xyz = (rs.rand(M, 3) * np.array([side, side, 4.0])).astype(np.float32)
        scenes.append((xyz, None, rs.randint(0, C, M).astype(np.int64)))
    return scenes


def main():
    assert torch.cuda.is_available(), "scenes_vote_bench measures the MI355X"
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    torch.manual_seed(0)
    model = Model(RandLANetSettings(n_classes=C, n_points=N, n_neighbors=16, layer_sizes=[16, 64, 128, 256, 512]))
    step = model.module.infer_step(B, N)
    forwards = [0]
    inner = step.step

    def counted(perm):
        forwards[0] += 1
        return inner(perm)

    step.step = counted              # both paths run their forwards through this cached step
    res = {"device": torch.cuda.get_device_name(0), "n": N, "B": B, "classes": C, "scenes": S, "votes": 1, "rows": []}
    for name, lo, hi in (("small", 10000, 40000), ("mixed", 10000, 120000)):
        scenes = make_set(lo, hi, seed=lo + hi)
        points = sum(x.shape[0] for x, _, _ in scenes)
        row = {"set": name, "points": points, "below_n": sum(x.shape[0] < N for x, _, _ in scenes)}
        for together in (False, True):
            kw = dict(batch_size=B, pad_small_scenes=True, together=together, return_confusion=True)
            model.evaluate_scenes(scenes[:4], **kw)          # warm the call path
            best = None
            for _ in range(2):
                np.random.seed(0)
                forwards[0] = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, conf = model.evaluate_scenes(scenes, **kw)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            assert int(conf.sum()) == points
            key = "together" if together else "loop"
            row[key + "_passes"] = forwards[0]
            row[key + "_s"] = round(best, 4)
        row["speedup"] = round(row["loop_s"] / row["together_s"], 2)
        res["rows"].append(row)
    assert list(model.module._infer_steps) == [(B, N)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
