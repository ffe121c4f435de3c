#!/usr/bin/env python3
"""Generates the golden fixtures in this directory FROM THE REFERENCE ITSELF.

Runs only in the build container (needs /root/reference and oracle/_ref/knn_tpk.so, the
reference's own C++ KNN built by oracle/build_ref.sh).  Fixtures are data only - inputs and
the reference's outputs; no reference source is stored.  Weights come from
oracle/init_formula.py, so they are not stored either.

How the reference is run ("PyTorch-CPU + C++ KNN"):
  * `import randlanet` from /root/reference needs two packages this image lacks; both get
    inert placeholders in sys.modules: `faiss` (knn.py:3; never called here) and
    `torch.utils.tensorboard` (trainer.py:11; SummaryWriter is never constructed here).
  * settings.knn = "approximate" and randlanet.utils.modules.knn_approximate is replaced by
    the reference's own compiled knn_tpk.knn - the contract of KNN.forward
    (modules.py:139-144) and the intent of its commented-out kdtree branch (modules.py:135-138).
    So every neighbour index / distance in the fixtures is produced by reference code.

Usage:  python tests/golden/make_golden.py            (writes *.npz / *.json next to itself)
"""
import json
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REF_ROOT", "/root/reference")

import numpy as np
import torch

sys.path.insert(0, os.path.join(REPO, "oracle", "_ref"))
sys.path.insert(0, REPO)
import knn_tpk  # noqa: E402  (the reference's C++ KNN, compiled from /root/reference)

from oracle.init_formula import formula_state_dict  # noqa: E402


def _import_reference():
    faiss = types.ModuleType("faiss")  # inert: knn_approximate is replaced below
    sys.modules.setdefault("faiss", faiss)
    tb = types.ModuleType("torch.utils.tensorboard")

    class SummaryWriter:  # never constructed by this script
        def __init__(self, *a, **k):
            raise RuntimeError("tensorboard placeholder")

    tb.SummaryWriter = SummaryWriter
    sys.modules.setdefault("torch.utils.tensorboard", tb)
    sys.path.insert(0, REF)
    import randlanet  # noqa: F401
    from randlanet.utils import modules as M

    def knn_cpp(xyz, xyz_query, k):
        return knn_tpk.knn(xyz.contiguous().float().cpu(), xyz_query.contiguous().float().cpu(), k)

    M.knn_approximate = knn_cpp
    return M


M = _import_reference()
from randlanet.utils import losses as RL  # noqa: E402
from randlanet.utils import metrics as RM  # noqa: E402
from randlanet.utils.trainer import Trainer  # noqa: E402

torch.manual_seed(0)
DEV = torch.device("cpu")


def save(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB")


def mock_cloud(n, seed=0):
    files = sorted(f for f in os.listdir(os.path.join(REF, "data", "mock")) if f.endswith("_data.npy"))
    xyz = np.load(os.path.join(REF, "data", "mock", files[-1])).astype(np.float32)
    sel = np.random.RandomState(seed).choice(xyz.shape[0], n, replace=False)
    return np.ascontiguousarray(xyz[sel])


# --------------------------------------------------------------------------------- G1: KNN
def g1_knn():
    cases = {}

    def add(tag, support, query, k, data_tag=None):
        """data_tag: cases sharing one point set store it once under <data_tag>/support."""
        s = torch.from_numpy(support[None]).contiguous()
        q = torch.from_numpy(query[None]).contiguous()
        idx, d2 = knn_tpk.knn(s, q, k)
        data_tag = data_tag or tag
        cases[f"{data_tag}/support"] = support
        if query is not support:
            cases[f"{data_tag}/query"] = query
        cases[f"{tag}/data"] = np.array(data_tag)
        cases[f"{tag}/idx"] = idx[0].numpy().astype(np.int32)
        cases[f"{tag}/d2"] = d2[0].numpy()
        cases[f"{tag}/k"] = np.int32(k)

    rs = np.random.RandomState(0)
    for n in (64, 1000, 4096):
        pts = rs.uniform(0, 1, (n, 3)).astype(np.float32)
        for k in (1, 16, 32):
            add(f"uniform_n{n}_k{k}", pts, pts, k, f"uniform_n{n}")
    sup = rs.uniform(0, 1, (1024, 3)).astype(np.float32)
    qry = np.concatenate([sup, rs.uniform(0, 1, (3072, 3)).astype(np.float32)])
    add("cross_1nn", sup, qry, 1, "cross")
    add("cross_8nn", sup, qry, 8, "cross")
    mock = mock_cloud(4096)
    add("mock_k16", mock, mock, 16)
    # predict.py:23 warm-up shape: 30 base points sampled up to 2500 with duplicates
    base = rs.uniform(0, 1, (30, 3)).astype(np.float32)
    dup = base[np.r_[np.arange(30), rs.randint(0, 30, 2470)]]
    add("duplicates_k32", dup, dup, 32)
    g = np.arange(16, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    add("lattice_k16", lattice, lattice, 16)
    save("knn_cases.npz", **cases)


# ----------------------------------------------------------------------- helpers for models
def build_ref_net(n_classes, n_points, k, layer_sizes, n_features=0):
    s = M.RandLANetSettings(n_classes=n_classes, n_points=n_points, n_features=n_features,
                            n_neighbors=k, layer_sizes=list(layer_sizes), knn="approximate")
    net = M.RandLANet(s, DEV)
    sd = net.state_dict()
    net.load_state_dict(formula_state_dict([(k_, tuple(v.shape)) for k_, v in sd.items()]))
    return net


def dump_layout(tag, net):
    layout = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    with open(os.path.join(HERE, f"state_dict_{tag}.json"), "w") as f:
        json.dump(layout, f)
    n_param = sum(p.numel() for p in net.parameters())
    print(f"state_dict_{tag}.json: {len(layout)} entries, {n_param} parameters")


CONFIGS = {
    # tag: (n_classes, N, K, layer_sizes, B)
    "a4": (2, 2048, 16, [16, 64, 128, 256], 2),      # config A architecture, reduced N
    "s5": (13, 4096, 16, [8, 16, 32, 64, 128], 1),    # 5 encoder layers, 13 classes
    "p32": (2, 2500, 32, [16, 64, 128, 256], 1),     # train.py:50-51 settings
}


def make_input(tag, B, N, seed):
    rs = np.random.RandomState(seed)
    if tag == "p32":
        return mock_cloud(N, seed)[None].repeat(B, 0)
    return rs.uniform(0, 1, (B, N, 3)).astype(np.float32)


# ------------------------------------------------------------------ G2: eval-mode forward
def g2_net_eval():
    for tag, (C, N, K, layers, B) in CONFIGS.items():
        net = build_ref_net(C, N, K, layers).eval()
        dump_layout(tag, net)
        x = make_input(tag, B, N, 7)
        np.random.seed(0)
        perm = np.random.permutation(N)
        np.random.seed(0)
        with torch.no_grad():
            logits = net(torch.from_numpy(x))
        save(f"net_eval_{tag}.npz", input=x, permutation=perm.astype(np.int64),
             logits=logits.numpy(), meta=np.array([C, N, K, B] + list(layers), dtype=np.int64))


def g2_modules():
    """Single-module outputs (eval mode) for pinning the oracle restatement block by block."""
    out = {}
    rs = np.random.RandomState(3)
    B, N, K, d_in, d = 2, 256, 16, 8, 16
    xyz = rs.uniform(0, 1, (B, N, 3)).astype(np.float32)
    feats = rs.uniform(-1, 1, (B, d_in, N, 1)).astype(np.float32)
    lfa = M.LocalFeatureAggregation(d_in, d, K, DEV)
    sd = lfa.state_dict()
    lfa.load_state_dict(formula_state_dict([(k_, tuple(v.shape)) for k_, v in sd.items()], seed=77))
    lfa.eval()
    with torch.no_grad():
        y = lfa(torch.from_numpy(xyz), torch.from_numpy(feats), "approximate")
        idx, dist = lfa.knn(torch.from_numpy(xyz), torch.from_numpy(xyz), K, "approximate")
        rpe = lfa.rpe(torch.from_numpy(xyz), idx, dist)
        pool_in = torch.from_numpy(rs.uniform(-1, 1, (B, d, N, K)).astype(np.float32))
        pooled = lfa.pool1(pool_in)
    # the reference KNN's own squared distances: the `dist` channel of rpe is torch.sqrt of them, an op whose last bit
    # follows the code path MKL picks for the host CPU, so the test re-evaluates it from these on its own host
    knn_idx, knn_d2 = knn_tpk.knn(torch.from_numpy(xyz), torch.from_numpy(xyz), K)
    save("mod_blocks_knn.npz", idx=knn_idx.numpy(), d2=knn_d2.numpy())
    out.update(lfa_xyz=xyz, lfa_feats=feats, lfa_out=y.numpy(), rpe=rpe.numpy(),
               pool_in=pool_in.numpy(), pool_out=pooled.numpy(),
               lfa_layout=np.array(json.dumps([[k_, list(v.shape)] for k_, v in sd.items()])))
    # UpSampler variants (modules.py:416-456)
    f = torch.from_numpy(rs.uniform(-1, 1, (B, 5, 64, 1)).astype(np.float32))
    xyz_c, xyz_f = torch.from_numpy(xyz[:, :64].copy()), torch.from_numpy(xyz)
    for approach in ("nni", "nna", "idw", "isdw"):
        up = M.UpSampler(approach, DEV)
        with torch.no_grad():
            out[f"up_{approach}"] = up(f, xyz_c, xyz_f).numpy()
    out["up_feats"] = f.numpy()
    save("mod_blocks.npz", **out)


# ------------------------------------------------------------- G3: train mode, grads, Adam
def g3_train():
    C, N, K, layers, B = 3, 512, 8, [8, 16, 32, 32], 2
    net = build_ref_net(C, N, K, layers)
    dump_layout("t4", net)
    net.fc_end[2].p = 0.0          # neutralise Dropout (torch RNG is not part of the contract)
    net.train()
    rs = np.random.RandomState(11)
    x = rs.uniform(0, 1, (B, N, 3)).astype(np.float32)
    labels = (np.floor(x[..., 2] * C).clip(0, C - 1)).astype(np.int64)
    np.random.seed(5)
    perm = np.random.permutation(N)
    np.random.seed(5)
    crit = Trainer._get_loss("dice")
    logits = net(torch.from_numpy(x))
    loss = crit(logits, torch.from_numpy(labels))
    net.zero_grad()
    loss.backward()
    out = dict(input=x, labels=labels, permutation=perm.astype(np.int64), logits=logits.detach().numpy(),
               loss=np.float32(loss.item()), meta=np.array([C, N, K, B] + layers, dtype=np.int64))
    for name, p in net.named_parameters():
        out[f"grad/{name}"] = p.grad.numpy().copy()
    for name, b in net.named_buffers():
        if name.endswith("running_mean") or name.endswith("running_var"):
            out[f"buf/{name}"] = b.numpy().copy()
    # five Adam steps (trainer.py:78, 114-119), same batch, fresh permutation each forward
    net2 = build_ref_net(C, N, K, layers)
    net2.fc_end[2].p = 0.0
    net2.train()
    opt = torch.optim.Adam(net2.parameters(), lr=1e-2)
    np.random.seed(9)
    traj = []
    for _ in range(5):
        lg = net2(torch.from_numpy(x))
        ls = crit(lg, torch.from_numpy(labels))
        opt.zero_grad()
        ls.backward()
        opt.step()
        traj.append(ls.item())
    out["adam_losses"] = np.array(traj, dtype=np.float32)
    out["adam_final_fc_end3_w"] = net2.state_dict()["fc_end.3.conv.weight"].numpy().copy()
    save("train_t4.npz", **out)


# ------------------------------------------------------------------ G4: losses and metrics
def g4_loss_metrics():
    rs = np.random.RandomState(21)
    out = {}
    for tag, (B, C, N) in {"c2": (2, 2, 300), "c5": (3, 5, 200)}.items():
        logits = rs.normal(0, 2, (B, C, N)).astype(np.float32)
        labels = rs.randint(0, C, (B, N)).astype(np.int64)
        if tag == "c5":
            labels[labels == 3] = 1      # class 3 absent from labels
            logits[:, 4] = -50.0         # class 4 never predicted
        out[f"{tag}/logits"], out[f"{tag}/labels"] = logits, labels
        lt, yt = torch.from_numpy(logits).requires_grad_(True), torch.from_numpy(labels)
        for name in ("cross_entropy", "focal", "dice", "tversky", "focal_tversky"):
            crit = Trainer._get_loss(name)
            l = crit(lt, yt)
            (g,) = torch.autograd.grad(l, lt)
            out[f"{tag}/{name}"] = np.float32(l.item())
            out[f"{tag}/{name}_grad"] = g.numpy()
        oa, pca = RM.accuracy(lt.detach(), yt)
        miou, pci = RM.iou(lt.detach(), yt)
        out[f"{tag}/oa"], out[f"{tag}/pca"] = np.float64(oa), np.array(pca)
        out[f"{tag}/miou"], out[f"{tag}/pci"] = np.float64(miou), np.array(pci)
    save("loss_metrics.npz", **out)


# ------------------------------------------------- G5: model zip + Model.predict (facade)
def synthetic_labels(xyz, n_classes):
    """Deterministic, spatially coherent labels for the unlabeled mock clouds: class grows with
    the distance from the cloud centroid, class 0 beyond the median radius."""
    c = xyz.mean(0, keepdims=True)
    r = np.linalg.norm(xyz - c, axis=1)
    med = np.median(r)
    lab = 1 + np.floor((n_classes - 1) * r / med).astype(np.int64)
    return np.where(r < med, np.clip(lab, 1, n_classes - 1), 0).astype(np.int64)


def g5_model_zip():
    from pathlib import Path
    from randlanet import Model, RandLANetSettings
    s = RandLANetSettings(n_classes=2, n_points=600, n_neighbors=8, layer_sizes=[8, 16, 32, 32],
                          knn="approximate", upsampling="nni")
    model = Model(s, use_gpu=False)
    sd = model.module.state_dict()
    model.module.load_state_dict(formula_state_dict([(k_, tuple(v.shape)) for k_, v in sd.items()], seed=5))
    model.module.eval()
    zip_path = Path(HERE) / "ref_model_small.zip"
    model.save(zip_path)
    cloud = mock_cloud(5000, seed=2)
    out = {}
    for up in ("nni", "idw"):
        model.settings.upsampling = up
        model._upsampler = M.UpSampler(up, DEV)
        np.random.seed(123)
        out[f"conf_{up}"] = np.asarray(model.predict(cloud))
    np.random.seed(123)
    raw = model.predict(cloud[:600], prepostprocess=False)
    out["conf_raw"] = np.asarray(raw.numpy() if hasattr(raw, "numpy") else raw)
    save("model_predict.npz", cloud=cloud, **out)
    print(f"ref_model_small.zip: {os.path.getsize(zip_path) / 1024:.0f} KiB")


# ------------------------------------------------------- G6: short training run (mIoU)
def g6_training_run():
    from randlanet import AugmentationSettings, Model, RandLANetSettings, TrainingSettings
    C, n_pts = 3, 1024
    clouds = []
    for i in range(12):
        xyz = mock_cloud(3000, seed=10 + i)
        clouds.append((xyz, np.zeros((3000, 0), np.float32), synthetic_labels(xyz, C)))
    train, val = clouds[:8], clouds[8:]
    torch.manual_seed(0)
    np.random.seed(0)
    s = RandLANetSettings(n_classes=C, n_points=n_pts, n_neighbors=16, layer_sizes=[8, 16, 32, 32],
                          knn="approximate")
    model = Model(s, use_gpu=False)
    model.module.fc_end[2].p = 0.0          # Dropout draws from torch's device RNG: not comparable
    hist = []
    ts = TrainingSettings(epochs=6, batch_size=4, learning_rate=1e-2, early_stopping=False)
    model.train(train, val, ts, AugmentationSettings(), None, ["bg", "a", "b"],
                callbacks=[lambda e, m: hist.append([m["loss"], m["mIoU"], m["val_loss"], m["val_mIoU"]])])
    final = model.evaluate(val, ["bg", "a", "b"], batch_size=4)
    save("train_run.npz", clouds=np.stack([c[0] for c in clouds]).astype(np.float32),
         labels=np.stack([c[2] for c in clouds]).astype(np.int8), history=np.array(hist, dtype=np.float64),
         final=np.array([final["loss"], final["OA"], final["mAcc"], final["mIoU"]], dtype=np.float64))
    print("history", np.round(np.array(hist), 4).tolist(), "final", final)


def g6s_training_seeds(n_seeds=64, first_seed=0, out_name="train_seeds.npz"):
    """The G6 run repeated by the REFERENCE trainer over `n_seeds` (torch seed, numpy seed) pairs on the clouds of
    train_run.npz: the distribution of the final validation mIoU (and of the whole per-epoch history) that the HIP
    path's same-seed runs are compared with (north_star: mIoU parity; reference evaluation loop trainer.py:271-367,
    per-batch averaging metrics.py:149-151, 10 seeded passes metrics.py:239-242)."""
    from randlanet import AugmentationSettings, Model, RandLANetSettings, TrainingSettings
    z = np.load(os.path.join(HERE, "train_run.npz"))
    C, n_pts = 3, 1024
    clouds = [(xyz, np.zeros((xyz.shape[0], 0), np.float32), lab.astype(np.int64)) for xyz, lab in zip(z["clouds"], z["labels"])]
    train, val = clouds[:8], clouds[8:]
    hists, finals = [], []
    for seed in range(first_seed, first_seed + n_seeds):
        torch.manual_seed(seed)
        np.random.seed(seed)
        s = RandLANetSettings(n_classes=C, n_points=n_pts, n_neighbors=16, layer_sizes=[8, 16, 32, 32], knn="approximate")
        model = Model(s, use_gpu=False)
        model.module.fc_end[2].p = 0.0          # Dropout draws from torch's device RNG: not comparable
        hist = []
        ts = TrainingSettings(epochs=6, batch_size=4, learning_rate=1e-2, early_stopping=False)
        model.train(train, val, ts, AugmentationSettings(), None, ["bg", "a", "b"],
                    callbacks=[lambda e, m: hist.append([m["loss"], m["mIoU"], m["val_loss"], m["val_mIoU"]])])
        hists.append(hist)
        finals.append(hist[-1][3])
        print(f"seed {seed}: val_mIoU per epoch {np.round(np.array(hist)[:, 3], 4).tolist()}", flush=True)
    finals = np.array(finals)
    save(out_name, seeds=np.arange(first_seed, first_seed + n_seeds), histories=np.array(hists, dtype=np.float64), final_val_miou=finals)
    print(f"final val_mIoU over {n_seeds} seeds: mean {finals.mean():.4f} std {finals.std(ddof=1):.4f} "
          f"SE {finals.std(ddof=1) / np.sqrt(n_seeds):.4f}")


# ------------------------------------- G8: same-weights evaluation (the 0.1-pt mIoU criterion)
def g8_eval_parity(epochs=40):
    """north_star: "mIoU within 0.1 pt of the reference on the held-out mock set".  A training RUN cannot resolve 0.001
    (train_seeds.npz: sigma over seeds 0.11), an EVALUATION can: it is deterministic on both sides.  The REFERENCE trains
    on the 8 training sub-samples of train_run.npz for `epochs` epochs and saves its zip; the reference's own
    Model.evaluate (trainer.py:271-367: 10 seeded passes, per-batch averaging metrics.py:149-151, pass averaging
    metrics.py:239-242) on the 4 held-out sub-samples is stored for three batch sizes.  The HIP path loads the same zip
    and must reproduce every number within 0.001 (tests/test_model_gpu.py::test_same_weights_evaluation_matches_reference).
    Two models: the 16-neighbour one (fused pooling kernels) and one with train.py's 32 neighbours / 2 classes."""
    from pathlib import Path
    from randlanet import AugmentationSettings, Model, RandLANetSettings, TrainingSettings
    z = np.load(os.path.join(HERE, "train_run.npz"))
    out = {}
    for tag, C, K, n_pts, names in (("k16c3", 3, 16, 1024, ["bg", "a", "b"]), ("k32c2", 2, 32, 2048, ["bg", "tip"])):
        clouds = [(xyz, np.zeros((xyz.shape[0], 0), np.float32), np.minimum(lab.astype(np.int64), C - 1))
                  for xyz, lab in zip(z["clouds"], z["labels"])]
        train, val = clouds[:8], clouds[8:]
        torch.manual_seed(1)
        np.random.seed(1)
        s = RandLANetSettings(n_classes=C, n_points=n_pts, n_neighbors=K, layer_sizes=[8, 16, 32, 32], knn="approximate")
        model = Model(s, use_gpu=False)
        hist = []
        ts = TrainingSettings(epochs=epochs, batch_size=4, learning_rate=1e-2, early_stopping=False)
        model.train(train, val, ts, AugmentationSettings(), None, names,
                    callbacks=[lambda e, m: hist.append([m["loss"], m["mIoU"], m["val_loss"], m["val_mIoU"]])])
        model.save(Path(HERE) / f"ref_trained_{tag}.zip")
        keys = None
        for bs in (16, 4, 1):
            d = model.evaluate(val, names, batch_size=bs, include_stdev=True)
            keys = list(d.keys())
            out[f"{tag}/eval_bs{bs}"] = np.array([[v[0], v[1]] for v in d.values()], dtype=np.float64)
            print(tag, "bs", bs, {k: round(v[0], 5) for k, v in d.items()})
        d = model.evaluate(val, names, batch_size=1, postprocess=True)
        out[f"{tag}/eval_post_bs1"] = np.array(list(d.values()), dtype=np.float64)
        out[f"{tag}/keys"] = np.array(json.dumps(keys))
        out[f"{tag}/history"] = np.array(hist, dtype=np.float64)
        print(tag, "val_mIoU per epoch", np.round(np.array(hist)[:, 3], 4).tolist())
        print(f"ref_trained_{tag}.zip: {os.path.getsize(Path(HERE) / f'ref_trained_{tag}.zip') / 1024:.0f} KiB")
    save("eval_parity.npz", **out)


# --------------------------------------------------------------------- G7: input pipeline
def g7_pipeline():
    """The reference's own PointCloudPreprocessor / get_data_loader on small clouds."""
    from dataclasses import asdict
    from randlanet.utils.augmentation import AugmentationSettings
    from randlanet.utils.dataset import PointCloudPreprocessor, get_data_loader

    rs = np.random.RandomState(77)
    out = {}
    custom = AugmentationSettings(jitter_variance=0.03, jitter_limit=0.02, scale_limit=0.3, shift_limit=0.25,
                                  rotation_angle_variances=(0.2, 0.05, 0.4), rotation_angle_limits=(0.1, 0.3, 0.5))
    cases = [   # tag, n_src, dtype, F, n_sample, consistent, augmentation, normalization, numpy seed
        ("a", 3000, np.float32, 2, 2048, False, AugmentationSettings(), None, 5),
        ("b", 1500, np.float32, 0, 2048, True, custom, "mean", 6),
        ("c", 2500, np.float64, 1, 1024, True, None, "max", 7),
        ("d", 2200, np.float32, 0, 2048, False, custom, "stdev", 8),
        ("e", 2100, np.float64, 0, 512, False, AugmentationSettings(), "centre-only", 9),
    ]
    meta = []
    for tag, n_src, dt, F, n, cons, aug, norm, seed in cases:
        xyz = mock_cloud(n_src, seed=seed).astype(dt)
        feats = rs.rand(n_src, F).astype(np.float32)
        labels = rs.randint(0, 3, n_src).astype(np.int64)
        pre = PointCloudPreprocessor([(xyz, feats, labels)], n, consistent_sampling=cons, augmentation_settings=aug,
                                     normalization=norm)
        np.random.seed(seed)
        inp, lab, _ = pre[0]
        after = np.random.get_state()[1][:4].astype(np.int64)     # where the reference left the global stream
        out[f"{tag}_xyz"], out[f"{tag}_features"], out[f"{tag}_labels"] = xyz, feats, labels
        out[f"{tag}_out_input"], out[f"{tag}_out_labels"] = inp.numpy(), lab.numpy()
        out[f"{tag}_state_after"] = after
        meta.append(dict(tag=tag, n_sample=n, consistent=cons, normalization=norm, seed=seed,
                         augmentation=None if aug is None else asdict(aug)))
    # a shuffled, augmented epoch through the reference's DataLoader (batch composition + stream order)
    ds = [(mock_cloud(1200 + 100 * i, seed=20 + i), np.zeros((1200 + 100 * i, 0), np.float32),
           rs.randint(0, 2, 1200 + 100 * i).astype(np.int64)) for i in range(5)]
    torch.manual_seed(3)
    np.random.seed(4)
    loader = get_data_loader(ds, 1024, 2, shuffle=True, consistent_sampling=False, augmentation_settings=AugmentationSettings())
    order, batches, blabels = [], [], []
    for inp, lab, idx in loader:
        order.append(np.pad(idx.numpy(), (0, 2 - len(idx)), constant_values=-1))
        batches.append(np.concatenate([inp.numpy(), np.zeros((2 - inp.shape[0],) + tuple(inp.shape[1:]), np.float32)]))
        blabels.append(np.concatenate([lab.numpy(), np.zeros((2 - lab.shape[0], lab.shape[1]), np.int64)]))
    for i, c in enumerate(ds):
        out[f"loader_xyz{i}"], out[f"loader_labels{i}"] = c[0], c[2].astype(np.int8)
    out["loader_order"], out["loader_inputs"], out["loader_out_labels"] = np.stack(order), np.stack(batches), np.stack(blabels).astype(np.int8)
    save("pipeline.npz", **out)
    with open(os.path.join(HERE, "pipeline_cases.json"), "w") as fh:
        json.dump(meta, fh, indent=1)


if __name__ == "__main__":
    which = sys.argv[1:] or ["g1", "g2", "g2m", "g3", "g4", "g5", "g6", "g7"]
    if "g7" in which:
        g7_pipeline()
    if "g1" in which:
        g1_knn()
    if "g2" in which:
        g2_net_eval()
    if "g2m" in which:
        g2_modules()
    if "g3" in which:
        g3_train()
    if "g4" in which:
        g4_loss_metrics()
    if "g5" in which:
        g5_model_zip()
    if "g6" in which:
        g6_training_run()
    if "g6s" in which:
        g6s_training_seeds()
    if "g6s2" in which:     # a second, independent seed set (is the paired drift of the first one a property or noise?)
        g6s_training_seeds(64, 64, "train_seeds2.npz")
    if "g8" in which:
        g8_eval_parity()
