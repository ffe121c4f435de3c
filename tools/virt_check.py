#!/usr/bin/env python3
"""Virtual rpe branch vs the stored one (ops.virtual_rpe_supported forced to False) on a whole training step at benchmark size: loss and every
parameter gradient of the two schedules side by side - localises a defect of the virtual kernels without the CPU oracle.
    python tools/virt_check.py [B] [N]"""
import os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "3d_recognizer_amd"))
import numpy as np, torch
from randlanet import _ops as ops
from randlanet._train import TrainStep
from randlanet.utils.modules import RandLANet, RandLANetSettings

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
N = int(sys.argv[2]) if len(sys.argv) > 2 else 40960
dev = torch.device("cuda")
torch.manual_seed(23)
net = RandLANet(RandLANetSettings(n_classes=2, n_points=N, n_neighbors=16, layer_sizes=[16, 64, 128, 256], knn="kdtree"), dev)
net.fc_end[2].p = 0.0
sd = {k: v.clone() for k, v in net.state_dict().items()}
rs = np.random.RandomState(6)
x = rs.uniform(0, 1, (B, N, 3)).astype(np.float32)
y = (np.linalg.norm(x - 0.5, axis=-1) < 0.3).astype(np.int64)
perm = np.random.RandomState(9).permutation(N)
res = {}
virtual_rpe_supported = ops.virtual_rpe_supported
for virt in (True, False):
    ops.virtual_rpe_supported = virtual_rpe_supported if virt else (lambda *a, **k: False)
    net.load_state_dict(sd)
    net.train()
    st = TrainStep(net, B, N, loss="dice", use_graph=False)
    st.set_batch(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
    st.perm.copy_(torch.from_numpy(perm).to(dev))
    st._fwd_bwd()
    torch.cuda.synchronize()
    res[virt] = (float(st.out[0]), {n: st.flat.grads[n].clone() for n, _ in net.named_parameters()})
print("loss virtual", res[True][0], "stored", res[False][0])
rows = []
for n, g in res[True][1].items():
    r = res[False][1][n]
    sc = float(r.abs().max())
    rows.append((float((g - r).abs().max()) / max(sc, 1e-20), n, sc))
bad = 0
for e, n, sc in sorted(rows, reverse=True)[:25]:
    print(f"{n:48s} rel err {e:.3e}  scale {sc:.3e}")
print("parameters with rel err > 5e-2:", sum(1 for e, n, sc in rows if e > 5e-2 and not n.endswith('conv.bias')), "of", len(rows))
