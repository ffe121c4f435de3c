"""Generator of tests/golden/step_trace.json, and the case runner tests/test_schedule_gpu.py shares with it.

What is pinned, per case: the host-side launch sequence of one eager pass - every launch of the path goes through
`_hip.check(rc, "rl_xxx")`, so a wrapper around it sees all of them, together with the encoder-level tag (`_ops.LEVEL`) the
kernel timer would file the launch under - and SHA-256 digests of what the pass leaves behind (loss record, gradients,
parameters, logits).  Everything is seed-fixed and host-side: weights by oracle.init_formula over the net's own state_dict
shapes, inputs from np.random.RandomState.  Only names that every revision of the schedule has are used, so the file generated
at one commit says whether another commit launches and computes the same.

    python tests/golden/make_step_trace.py [out.json]        (on the MI355X; default: tests/golden/step_trace.json)
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (REPO, os.path.join(REPO, "3d_recognizer_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

LAYERS = [16, 64, 128, 256]
# name -> (K, C, F, B, N, p_drop, fused head allowed)
CASES = {
    "A": dict(K=16, C=2, F=0, B=2, N=4096, p=0.5, fused=True),     # virtual rpe, fused + un-fused pools, band sort, fused head
    "B": dict(K=16, C=13, F=2, B=3, N=1500, p=0.5, fused=True),    # cin != 3, 1-D perm, explicit mask, separate head launches
    "C": dict(K=32, C=3, F=0, B=1, N=2048, p=0.5, fused=False),    # stored rpe at every level, Philox dropout record
    "D": dict(K=32, C=3, F=0, B=1, N=2048, p=0.0, fused=False),    # fc_end.1 feeds fc_end.3: no dropout record
    "E": dict(K=16, C=2, F=0, B=2, N=4096, p=0.5, fused=True),     # eval: fold table built, then grouped pre-folds
}


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def tracer(calls: list):
    """The wrapper to put in place of _hip.check: appends [entry point, level tag] to `calls`, then checks as before."""
    from randlanet import _hip as H
    from randlanet import _ops as ops
    orig = H.check

    def check(rc, what=""):
        calls.append([what, ops.LEVEL])
        return orig(rc, what)
    return check


def run_case(name: str, calls: list) -> dict:
    """Runs case `name`; `calls` is the list the installed tracer() appends to.  Returns the fixture entry."""
    from oracle.init_formula import formula_state_dict
    from randlanet import _ops as ops
    from randlanet._train import TrainStep
    from randlanet.utils.modules import RandLANet, RandLANetSettings
    c = CASES[name]
    K, C, F, B, N, p = c["K"], c["C"], c["F"], c["B"], c["N"], c["p"]
    dev = torch.device("cuda")
    no_fused = ops.NO_FUSED_HEAD
    ops.NO_FUSED_HEAD = not c["fused"]
    try:
        torch.manual_seed(1234)                   # (the engine takes its Dropout seed from torch's seed when it is built)
        net = RandLANet(RandLANetSettings(n_classes=C, n_points=N, n_features=F, n_neighbors=K, layer_sizes=list(LAYERS)), dev)
        net.load_state_dict(formula_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], seed=99))
        net.fc_end[2].p = p
        rs = np.random.RandomState(7)
        x = torch.from_numpy(rs.uniform(0, 1, (B, N, 3 + F)).astype(np.float32)).to(dev)
        y = torch.from_numpy(np.floor(rs.uniform(0, 1, (B, N)) * C).clip(0, C - 1).astype(np.int64)).to(dev)
        perms = [rs.permutation(N) for _ in range(2)]
        out = {}
        if name == "E":
            net.eval()
            eng = net.engine()
            for i, perm in enumerate(perms):
                k0 = len(calls)
                with torch.no_grad():
                    logits, _ = eng.forward(x, torch.from_numpy(perm).to(dev), False)
                torch.cuda.synchronize()
                out[f"calls{i + 1}"], out[f"logits{i + 1}"] = calls[k0:], sha(logits)
        elif name == "B":
            net.train()
            eng = net.engine()
            kind, alpha, gamma = ops.LOSS_KINDS["dice"]
            keep = torch.from_numpy((rs.uniform(size=(B * N, 32)) < 1.0 - p).astype(np.uint8)).to(dev)
            for i, perm in enumerate(perms):
                k0 = len(calls)
                grads = {n: torch.zeros_like(q) for n, q in net.named_parameters()}
                logits, ctx = eng.forward(x, torch.from_numpy(perm).to(dev), True, p, keep_mask=keep)
                rec, work = ops.loss_forward(logits, y, kind, alpha, gamma, True)
                eng.backward(ctx, ops.loss_backward(logits, y, kind, alpha, gamma, True, work), grads)
                torch.cuda.synchronize()
                if i == 0:
                    out["calls"], out["loss1"] = calls[k0:], sha(rec)
                out[f"grad{i + 1}"] = sha(torch.cat([g.reshape(-1) for g in grads.values()]))
        else:
            net.train()
            step = TrainStep(net, B, N, loss="dice", lr=1e-2, use_graph=False)
            step.set_batch(x, y)
            torch.cuda.synchronize()
            k0 = len(calls)
            step.step(perms[0])
            torch.cuda.synchronize()
            out["calls"], out["loss1"], out["grad1"] = calls[k0:], sha(step.out), sha(step.flat.grad)
            step.step(perms[1])
            torch.cuda.synchronize()
            out["param2"] = sha(step.flat.param)
        return out
    finally:
        ops.NO_FUSED_HEAD = no_fused


def main() -> None:
    from randlanet import _hip as H
    dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "step_trace.json")
    calls: list = []
    orig = H.check
    H.check = tracer(calls)
    try:
        fixture = {name: run_case(name, calls) for name in CASES}
    finally:
        H.check = orig
    with open(dest, "w") as f:
        json.dump(fixture, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    for name, ent in fixture.items():
        print(name, {k: (len(v) if isinstance(v, list) else v[:12]) for k, v in ent.items()})


if __name__ == "__main__":
    main()
