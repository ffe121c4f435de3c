"""Host-side contract of the drop-in modules (no GPU): settings dataclass, state_dict layout
against the reference's (tests/golden/state_dict_*.json), error behaviour."""
import json

import numpy as np
import pytest
import torch


def _net(C, N, K, layers, F=0):
    from randlanet.utils.modules import RandLANet, RandLANetSettings
    s = RandLANetSettings(n_classes=C, n_points=N, n_features=F, n_neighbors=K, layer_sizes=list(layers))
    return RandLANet(s, torch.device("cpu"))


@pytest.mark.parametrize("tag", ["a4", "s5", "p32", "t4"])
def test_state_dict_layout_equals_reference(golden_dir, tag):
    layout = json.load(open(f"{golden_dir}/state_dict_{tag}.json"))
    z = np.load(f"{golden_dir}/{'train_t4' if tag == 't4' else 'net_eval_' + tag}.npz")
    C, N, K, B, *layers = [int(v) for v in z["meta"]]
    sd = _net(C, N, K, layers).state_dict()
    assert [(k, list(v.shape)) for k, v in sd.items()] == [(k, list(s)) for k, s in layout]


def test_settings_contract():
    from randlanet.utils.modules import RandLANetSettings
    s = RandLANetSettings(n_classes=2)
    assert (s.n_points, s.n_features, s.n_neighbors, s.decimation) == (10000, 0, 32, 4)
    assert s.layer_sizes == [16, 64, 128, 256] and s.knn == "approximate" and s.upsampling == "nni"
    with pytest.raises(AssertionError, match="knn value"):
        RandLANetSettings(n_classes=2, knn="brute")
    with pytest.raises(AssertionError, match="upsampling value"):
        RandLANetSettings(n_classes=2, upsampling="linear")
    s.update(n_points=5, bogus=1)
    assert s.n_points == 5 and not hasattr(s, "bogus")
    from dataclasses import asdict
    assert RandLANetSettings(**json.loads(json.dumps(asdict(s)))) == s      # Model.save/load round trip


def test_same_seed_same_default_init_order():
    """Registration order follows the reference, so the parameter count per config matches."""
    net = _net(2, 40960, 16, [16, 64, 128, 256])
    assert sum(p.numel() for p in net.parameters()) == 1322666
    net = _net(13, 65536, 16, [16, 64, 128, 256, 512])
    assert sum(p.numel() for p in net.parameters()) == 5337109
    assert net._min_n_points == 4096


def test_forward_asserts_and_no_cpu_path():
    from randlanet import _hip
    net = _net(2, 2048, 16, [16, 64, 128, 256])
    with pytest.raises(AssertionError, match=r"Input should have shape \(B, N, 3 \+ F\)!"):
        net(torch.zeros(1, 2048, 4))
    with pytest.raises(AssertionError, match="at least 1024 points"):
        net(torch.zeros(1, 100, 3))
    # a module placed on the CPU device: training is refused, eval runs the host path - which lives in the same
    # library (rl_knn_f32_cpu): without librandla_hip.so it fails loudly, there is no pure-Python stand-in
    with pytest.raises(_hip.HipKernelError, match="training runs on an MI355X"):
        net(torch.zeros(1, 2048, 3))
    net.eval()
    lib, path = _hip._LIB, _hip._LIB_PATH
    try:
        _hip._LIB, _hip._LIB_PATH = None, "/nonexistent/librandla_hip.so"
        with pytest.raises(_hip.HipKernelError, match="no fallback"):
            net(torch.rand(1, 2048, 3))
    finally:
        _hip._LIB, _hip._LIB_PATH = lib, path
    assert net(torch.rand(1, 2048, 3)).shape == (1, 2, 2048)
    with pytest.raises(_hip.HipKernelError, match="runs on an MI355X"):
        net.encoder[0].mlp1(torch.zeros(1, 8, 4, 1))


def test_import_creates_no_gpu_context_and_exports_the_reference_names():
    """train.py spawns its worker (reference train.py:108-115): importing must not touch HIP."""
    import subprocess, sys, os
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); import torch, randlanet; "
            "from randlanet import Model, RandLANetSettings, TrainingSettings, AugmentationSettings; "
            "assert sorted(randlanet.__all__) == ['AugmentationSettings', 'Model', 'RandLANetSettings', 'TrainingSettings']; "
            "assert not torch.cuda.is_initialized(); "
            "t = TrainingSettings(); a = AugmentationSettings(); "
            "assert (t.epochs, t.batch_size, t.learning_rate, t.learning_rate_decay, t.loss_function, t.early_stopping, "
            "t.early_stopping_patience) == (150, 8, 1e-2, 0.9, 'dice', True, 20); "
            "assert (a.jitter_variance, a.jitter_limit, a.scale_limit, a.shift_limit) == (0.01, 0.05, 0.2, 0.1); print('ok')"
            % os.path.join(repo, "3d_recognizer_amd"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


def test_sampling_and_augmentation_consume_the_rng_like_the_reference():
    """Seeded host glue (reference preprocessing.py:6-62, augmentation.py:143-167): `consistent` sampling is
    np.random.seed(0) + choice without touching the caller's stream; augmentation draws randn(N,3), uniform,
    3 x randn, uniform(3) in that order."""
    import numpy as np
    from randlanet.utils import preprocessing as P
    from randlanet.utils.augmentation import AugmentationSettings, perturbate_point_cloud
    np.random.seed(42)
    before = np.random.get_state()[1].copy()
    idx = P.sample_points(1000, 100, consistent=True)
    assert np.array_equal(np.random.get_state()[1], before)              # caller's stream untouched
    np.random.seed(0)
    assert np.array_equal(idx, np.random.choice(1000, 100, False, None))
    np.random.seed(0)
    up = P.sample_points(30, 100, consistent=True)                         # predict.py:23 warm-up: 30 -> n_points
    assert up.shape == (100,) and sorted(up[:30]) == list(range(30)) and up.max() < 30
    xyz = np.random.RandomState(1).uniform(0, 1, (50, 3))
    s = AugmentationSettings()
    np.random.seed(7)
    out = perturbate_point_cloud(xyz, s)
    np.random.seed(7)
    radius = np.mean(np.linalg.norm(xyz - xyz.mean(0, keepdims=True), axis=1))
    j = np.clip(radius * s.jitter_variance * np.random.randn(50, 3), -s.jitter_limit, s.jitter_limit) + xyz
    scale = np.random.uniform(1 - s.scale_limit, 1 + s.scale_limit)
    c = j.mean(0, keepdims=True)
    j = (j - c) * scale + c
    ang = [np.clip(0.06 * np.random.randn(), -0.18, 0.18) for _ in range(3)]
    cx, sx, cy, sy, cz, sz = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1]), np.cos(ang[2]), np.sin(ang[2])
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
         @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    c = j.mean(0, keepdims=True)
    j = (j - c) @ R.T + c
    radius = np.mean(np.linalg.norm(j - j.mean(0, keepdims=True), axis=1))
    j = j + radius * np.random.uniform(-s.shift_limit, s.shift_limit, 3)
    np.testing.assert_allclose(out, j, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------------
# The package's CPU device (reference model.py:38-40; config P = predict.py without a GPU): product-own host path.
def test_host_knn_twin_matches_reference_golden(golden_dir):
    """rl_knn_f32_cpu against the outputs of the COMPILED reference knn_tpk.knn (tests/golden/knn_cases.npz) under the
    parity rule of SURVEY 8a-3 (d2 bit-equal everywhere, index equal wherever the distance is unique in its row, ties in
    ascending index order), plus queries far outside the support's bounding box and k = Ns."""
    import numpy as np
    import torch
    from knn_parity import check_knn
    from randlanet._cpu import knn_host
    z = np.load(f"{golden_dir}/knn_cases.npz")
    tags = sorted({k.split("/")[0] for k in z.files if k.endswith("/idx")})
    assert len(tags) >= 14
    for t in tags:
        data = str(z[f"{t}/data"])
        sup = z[f"{data}/support"]
        qry = z[f"{data}/query"] if f"{data}/query" in z.files else sup
        idx, d2 = knn_host(torch.from_numpy(sup)[None], torch.from_numpy(qry)[None], int(z[f"{t}/k"]))
        frac = check_knn(idx[0].numpy(), d2[0].numpy(), z[f"{t}/idx"], z[f"{t}/d2"], sup, qry, expect_lowest_index=True)
        if t.startswith("uniform") or t.startswith("cross"):
            assert frac == 1.0, t
    rs = np.random.RandomState(3)
    s = torch.from_numpy(rs.normal(0, 1, (2, 700, 3)).astype(np.float32))
    q = torch.from_numpy(rs.normal(0, 4, (2, 300, 3)).astype(np.float32))        # most queries outside the support's box
    for k in (1, 8, 700):
        idx, d2 = knn_host(s, q, k)
        full = ((q[:, :, None, :] - s[:, None, :, :]) ** 2)
        ref = ((full[..., 0] + full[..., 1]) + full[..., 2])
        rd, ri = torch.sort(ref, dim=-1, stable=True)
        assert torch.equal(d2, rd[..., :k]) and torch.equal(idx, ri[..., :k])
    import pytest
    from randlanet import _hip
    with pytest.raises(_hip.HipKernelError, match="Not enough points"):
        knn_host(s[:, :5], q, 6)


def test_cpu_device_predict_matches_reference_golden(golden_dir):
    """Model.load(..., use_gpu=False).predict on the reference-written model zip: the confidences of the reference's own
    CPU run (tests/golden/model_predict.npz), through the host path (HostForward + rl_knn_f32_cpu + upsample_host)."""
    from pathlib import Path

    import numpy as np
    from randlanet import Model
    from randlanet.utils.modules import UpSampler
    z = np.load(f"{golden_dir}/model_predict.npz")
    model = Model.load(Path(golden_dir) / "ref_model_small.zip", use_gpu=False)
    assert model.device.type == "cpu" and model.module.device.type == "cpu"
    cloud = z["cloud"]
    for up in ("nni", "idw"):
        model.settings.upsampling = up
        model._upsampler = UpSampler(up, model.device)
        np.random.seed(123)
        conf = model.predict(cloud)
        assert isinstance(conf, np.ndarray) and conf.shape == (2, 5000)
        np.testing.assert_allclose(conf.sum(0), 1.0, atol=1e-5)
        bad = np.abs(conf - z[f"conf_{up}"]).max(0) > 1e-3          # exact-distance ties of the real depth cloud
        print(f"cpu device, {up}: {bad.mean():.4%} of the points differ by more than 1e-3 from the reference")
        assert bad.mean() < 0.02, (up, bad.mean())
    np.random.seed(123)
    raw = model.predict(cloud[:600], prepostprocess=False)
    assert np.mean(np.abs(np.asarray(raw) - z["conf_raw"]).max(0) > 1e-3) < 0.02
    # training stays a GPU matter, loudly
    import pytest
    import torch
    from randlanet import _hip
    model.module.train()
    with pytest.raises(_hip.HipKernelError, match="training runs on an MI355X"):
        model.module(torch.zeros(1, 600, 3))


def test_broaden_annotation_is_bit_identical_to_the_reference_loop():
    """the vectorised broaden_annotation against the reference's loop (dataset.py:8-18) restated with `bool`
    for the removed `np.bool` - float32 and float64 clouds, several radii, empty annotation."""
    import numpy as np
    from randlanet.utils.annotation import broaden_annotation

    def reference_loop(point_cloud, annotation, radius=0.01):
        output = []
        annotation_cloud = point_cloud[annotation.astype(bool)]
        for annotation_point in annotation_cloud:
            ds = np.abs(np.linalg.norm(annotation_point - point_cloud, axis=1))
            output.append(ds < radius)
        return np.logical_or.reduce(output).astype(np.uint8)

    rs = np.random.RandomState(0)
    for dtype in (np.float32, np.float64):
        cloud = rs.uniform(0, 0.3, (6000, 3)).astype(dtype)
        cloud[100:140] = cloud[100]                      # duplicates
        ann = (rs.uniform(size=6000) < 0.01).astype(np.uint8)
        for radius in (0.01, 0.02, 0.0):
            got, ref = broaden_annotation(cloud, ann, radius), reference_loop(cloud, ann, radius)
            assert got.dtype == ref.dtype == np.uint8 and np.array_equal(got, ref), (dtype, radius)
            if radius > 0:
                assert got.sum() > ann.sum()
    assert np.array_equal(broaden_annotation(cloud, np.zeros(6000, np.uint8)), reference_loop(cloud, np.zeros(6000, np.uint8)))


def test_reference_loads_a_zip_written_by_this_package(golden_dir, tmp_path):
    """SURVEY 8f-4, the reverse direction: a zip written by Model.save today holds what the reference's Model.load read from
    such a zip - the same settings, the same state_dict keys, shapes and (formula) values - and this package predicts the
    confidences the reference predicted from it (tests/golden/ref_loads_our_zip.npz, written by ref_loads_our_zip.py)."""
    import importlib.util
    import os
    import shutil
    spec = importlib.util.spec_from_file_location("ref_loads_our_zip", os.path.join(golden_dir, "ref_loads_our_zip.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    from oracle.init_formula import formula_state_dict
    zip_path, npz_path = tmp_path / "ours_model", tmp_path / "ours.npz"
    script.write(str(zip_path), str(npz_path))
    ref = np.load(f"{golden_dir}/ref_loads_our_zip.npz")
    shutil.unpack_archive(str(zip_path), str(tmp_path / "unpacked"), format="zip")
    with open(tmp_path / "unpacked" / "config") as f:
        assert json.load(f) == json.loads(str(ref["config"]))
    sd = torch.load(tmp_path / "unpacked" / "model", map_location="cpu")
    assert list(sd.keys()) == [str(k) for k in ref["keys"]]
    assert [list(v.shape) for v in sd.values()] == json.loads(str(ref["shapes"]))
    want = formula_state_dict([(k, tuple(v.shape)) for k, v in sd.items()], seed=9)
    for k in sd:
        assert torch.equal(sd[k], want[k]), k
    ours = np.load(npz_path)
    assert np.array_equal(ours["cloud"], ref["cloud"])
    err = np.abs(ours["conf"] - ref["conf"]).max()
    print(f"reference's confidences on our zip vs ours: max |difference| = {err:.2e}")
    assert err < 1e-4, err
