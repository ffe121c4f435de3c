"""Pins oracle/randlanet_oracle.py (the CPU restatement) against outputs of the real reference
generated in the build container (tests/golden/*.npz, see make_golden.py)."""
import json

import numpy as np
import pytest
import torch

from oracle import randlanet_oracle as O
from oracle.init_formula import formula_state_dict


def _params(golden_dir, tag, requires_grad=False):
    layout = json.load(open(f"{golden_dir}/state_dict_{tag}.json"))
    P = formula_state_dict([(k, tuple(s)) for k, s in layout])
    if requires_grad:
        for k, v in P.items():
            if v.is_floating_point() and "running" not in k:
                v.requires_grad_(True)
    return P, layout


@pytest.mark.parametrize("tag", ["a4", "s5", "p32"])
def test_layout_matches_reference(golden_dir, tag):
    z = np.load(f"{golden_dir}/net_eval_{tag}.npz")
    C, N, K, B, *layers = [int(v) for v in z["meta"]]
    layout = json.load(open(f"{golden_dir}/state_dict_{tag}.json"))
    mine = O.state_dict_layout(C, 0, layers)
    assert [(k, list(s)) for k, s in mine] == [(k, list(s)) for k, s in layout]


@pytest.mark.parametrize("tag", ["a4", "s5", "p32"])
def test_eval_logits_match_reference(golden_dir, tag):
    z = np.load(f"{golden_dir}/net_eval_{tag}.npz")
    C, N, K, B, *layers = [int(v) for v in z["meta"]]
    P, _ = _params(golden_dir, tag)
    with torch.no_grad():
        logits = O.forward(P, torch.from_numpy(z["input"]), z["permutation"],
                           layer_sizes=layers, n_neighbors=K, training=False)
    ref = z["logits"]
    assert logits.shape == ref.shape
    # identical ATen ops on identical inputs; allow only reduction-order noise.  The p32 case is
    # a real depth cloud with exact-distance ties, where the reference's kd-tree tie order may
    # pick a different (equally near) neighbour for a few points.
    err = np.abs(logits.numpy() - ref)
    if tag == "p32":
        assert np.mean(err > 1e-4) < 0.02, np.mean(err > 1e-4)
    else:
        assert err.max() <= 1e-5 * max(1.0, np.abs(ref).max()), err.max()


def test_blocks_match_reference(golden_dir):
    z = np.load(f"{golden_dir}/mod_blocks.npz")
    layout = json.loads(str(z["lfa_layout"]))
    P = formula_state_dict([(f"encoder.0.{k}", tuple(s)) for k, s in layout], seed=77)
    xyz = torch.from_numpy(z["lfa_xyz"])
    kz = np.load(f"{golden_dir}/mod_blocks_knn.npz")
    with torch.no_grad():
        idx, d2 = O.knn(xyz, xyz, 16)
        assert np.array_equal(idx.numpy(), kz["idx"]) and np.array_equal(d2.numpy(), kz["d2"])
        rpe = O.relative_position_encoding(xyz, idx, torch.sqrt(d2))
        assert torch.equal(rpe[:, :9], torch.from_numpy(z["rpe"][:, :9]))
        # the dist channel is the reference's torch.sqrt of its squared distances: that op's last bit follows the code path
        # MKL picks for the host CPU, so it is evaluated here, on this host, from the reference's own d2 ...
        assert torch.equal(rpe[:, 9], torch.sqrt(torch.from_numpy(kz["d2"])))
        # ... and the values the reference's host computed differ from it by no more than that last bit
        np.testing.assert_array_max_ulp(rpe[:, 9].numpy(), z["rpe"][:, 9], maxulp=1)
        pooled = O.attentive_pooling(P, "encoder.0.pool1", torch.from_numpy(z["pool_in"]))
        np.testing.assert_allclose(pooled.numpy(), z["pool_out"], rtol=1e-5, atol=1e-6)
        y = O.local_feature_aggregation(P, "encoder.0", xyz, torch.from_numpy(z["lfa_feats"]), 16)
        np.testing.assert_allclose(y.numpy(), z["lfa_out"], rtol=1e-5, atol=1e-6)
        f = torch.from_numpy(z["up_feats"])
        for approach in ("nni", "nna", "idw", "isdw"):
            up = O.upsample(f, xyz[:, :64].contiguous(), xyz, approach)
            np.testing.assert_allclose(up.numpy(), z[f"up_{approach}"], rtol=1e-5, atol=1e-6)
        assert np.array_equal(z["up_nna"], z["up_idw"])   # modules.py:434-437 quirk


def test_train_step_matches_reference(golden_dir):
    from oracle.loss_metrics_oracle import loss_by_name
    z = np.load(f"{golden_dir}/train_t4.npz")
    C, N, K, B, *layers = [int(v) for v in z["meta"]]
    P, layout = _params(golden_dir, "t4", requires_grad=True)
    buffers = {}
    logits = O.forward(P, torch.from_numpy(z["input"]), z["permutation"], layer_sizes=layers,
                       n_neighbors=K, training=True, dropout_p=0.0, buffers=buffers)
    np.testing.assert_allclose(logits.detach().numpy(), z["logits"], rtol=1e-4, atol=1e-5)
    loss = loss_by_name("dice", logits, torch.from_numpy(z["labels"]))
    assert abs(loss.item() - float(z["loss"])) < 1e-6
    loss.backward()
    for key in [k for k in z.files if k.startswith("grad/")]:
        name = key[5:]
        g, r = P[name].grad.numpy(), z[key]
        scale = max(np.abs(r).max(), 1e-6)
        assert np.abs(g - r).max() <= 2e-4 * scale + 1e-7, (name, np.abs(g - r).max(), scale)
    for key in [k for k in z.files if k.startswith("buf/")]:
        np.testing.assert_allclose(buffers[key[4:]].numpy(), z[key], rtol=1e-5, atol=1e-6)


def test_loss_metrics_match_reference(golden_dir):
    from oracle import loss_metrics_oracle as LM
    z = np.load(f"{golden_dir}/loss_metrics.npz")
    for tag in ("c2", "c5"):
        logits = torch.from_numpy(z[f"{tag}/logits"]).requires_grad_(True)
        labels = torch.from_numpy(z[f"{tag}/labels"])
        for name in ("cross_entropy", "focal", "dice", "tversky", "focal_tversky"):
            l = LM.loss_by_name(name, logits, labels)
            (g,) = torch.autograd.grad(l, logits)
            assert abs(l.item() - float(z[f"{tag}/{name}"])) < 1e-6, (tag, name)
            np.testing.assert_allclose(g.numpy(), z[f"{tag}/{name}_grad"], rtol=1e-4, atol=1e-8)
        oa, pca = LM.accuracy(z[f"{tag}/logits"], z[f"{tag}/labels"])
        miou, pci = LM.iou(z[f"{tag}/logits"], z[f"{tag}/labels"])
        assert abs(oa - float(z[f"{tag}/oa"])) < 1e-6
        np.testing.assert_allclose(pca, z[f"{tag}/pca"], atol=1e-6)
        assert abs(miou - float(z[f"{tag}/miou"])) < 1e-6
        np.testing.assert_allclose(pci, z[f"{tag}/pci"], atol=1e-6)
