#!/usr/bin/env python3
"""What the sorted loss costs per training step on one MI355X: _train.TrainStep (captured graph) at the metric's shape -
B = 8 clouds of N = 40960 points, the config-S network (13 classes, K = 16, layers [16, 64, 128, 256, 512]) - for
  dice            the default step: the head fused (rl_head_fwd / rl_head_bwd), no logits stored
  dice_unfused    the same loss through the separate launches (ops.NO_FUSED_HEAD): what storing the (B, C, N) logits costs
  lovasz          the Lovasz-Softmax loss (csrc/lovasz.hip): separate launches + softmax / keys, the radix sort of B*C*N keys,
                  the coefficient pass, the gradient pass
  lovasz_cross_entropy   ... plus the masked cross entropy's gradient pass
Every case is warmed up, then timed by device events around REPS replays per round, the cases alternated inside each of
ROUNDS rounds (>= 200 replays per case in all); per case the median round and the spread (min .. max) in ms per step, and
the sort's algorithmic bytes.  Prints one JSON line.  Not part of bench.py.  usage: python tools/lovasz_bench.py"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "3d_recognizer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from randlanet import _ops as ops  # noqa: E402
from randlanet._train import TrainStep  # noqa: E402
from randlanet.utils.modules import RandLANet, RandLANetSettings  # noqa: E402

N, B, C = 40960, 8, 13
ROUNDS, REPS = 6, 40
CASES = (("dice", "dice", False), ("dice_unfused", "dice", True), ("lovasz", "lovasz", False),
         ("lovasz_cross_entropy", "lovasz_cross_entropy", False))


def sort_bytes(B: int, C: int, N: int) -> int:
    """Bytes the sorted loss must move beyond the plain loss: keys written (8), per radix pass the keys read by the histogram
    (8) and keys + payload read and written by the scatter (24), the count pass (8), the coefficient pass (keys, payload,
    coefficient: 16), and the coefficient read by the backward (4) - per (class, point) pair."""
    passes = -(-(32 + C.bit_length()) // 8)
    return (8 + passes * 32 + 8 + 16 + 4) * B * C * N


def main():
    assert torch.cuda.is_available(), "lovasz_bench measures the MI355X"
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.uniform(0, 1, (B, N, 3)).astype(np.float32)).to(dev)
    y = torch.from_numpy(np.floor(rs.uniform(0, 1, (B, N)) ** 2 * C).clip(0, C - 1).astype(np.int64)).to(dev)
    perms = [rs.permutation(N) for _ in range(8)]
    steps = {}
    for tag, loss, unfused in CASES:
        torch.manual_seed(0)
        net = RandLANet(RandLANetSettings(n_classes=C, n_points=N, n_neighbors=16, layer_sizes=[16, 64, 128, 256, 512]), dev)
        net.train()
        step = TrainStep(net, B, N, loss=loss, use_graph=True)
        step.set_batch(x, y)
        ops.NO_FUSED_HEAD = unfused
        try:
            step.capture()
        finally:
            ops.NO_FUSED_HEAD = False
        for k in range(10):                                      # warm-up replays
            step.step(perms[k % len(perms)])
        torch.cuda.synchronize()
        steps[tag] = step
    times = {tag: [] for tag in steps}
    for _ in range(ROUNDS):
        for tag, step in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(REPS):
                step.step(perms[k % len(perms)])
            e1.record()
            torch.cuda.synchronize()
            times[tag].append(e0.elapsed_time(e1) / REPS)
    res = {"device": torch.cuda.get_device_name(0), "B": B, "N": N, "classes": C, "arithmetic": ops.get_wide_gemm(),
           "replays_per_case": ROUNDS * REPS, "sort_bytes_per_step": sort_bytes(B, C, N), "cases": {}}
    for tag, t in times.items():
        res["cases"][tag] = {"step_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                             "loss": round(float(steps[tag].out[0]), 6)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
