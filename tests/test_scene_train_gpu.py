"""Model.train_scenes on the MI355X: the rl_scenes_* kernels against their numpy twin (utils/scene.py scenes_crop) bit for
bit, one scene against rl_scene_crop, the scene crop loader against a host restatement, no host synchronisation while a
batch is prepared, and a tiny end-to-end training run."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _xyz(rs, M, lattice):
    if lattice:             # coarse lattice (many equal distances) with a quarter of the points duplicated
        ext = max(4.0, round(M ** (1 / 3)))
        x = np.floor(rs.uniform(0, ext, (M, 3))).astype(np.float32) * np.float32(0.25)
        x[rs.randint(0, M, M // 4)] = x[rs.randint(0, M, M // 4)]
        return x
    return rs.uniform(-3, 3, (M, 3)).astype(np.float32)


# name: (scene sizes, n, F, centre noise, lattice coordinates, crops); every case with several scenes has one of
# exactly n points
CASES = {
    "one": ([60000], 4096, 0, 0.0, True, 10),
    "seven": ([2048, 9000, 30000, 2500, 60000, 4000, 12000], 2048, 2, 0.05, True, 14),
    "fifty": (None, 1000, 0, 0.2, False, 20),
    "3M": ([40960, 1400000, 1000000, 559040], 40960, 1, 0.0, True, 6),
}


@pytest.mark.parametrize("case", list(CASES))
def test_scenes_crop_bitwise_twin(case):
    from randlanet import _ops as ops
    from randlanet.utils import scene
    sizes, n, F, noise, lattice, crops = CASES[case]
    rs = np.random.RandomState(len(case))
    if sizes is None:
        sizes = [int(v) for v in rs.randint(1000, 6000, 50)]
        sizes[17] = n
    xyz = np.concatenate([_xyz(rs, M, lattice) for M in sizes])
    T = xyz.shape[0]
    cloud = np.concatenate([xyz, rs.standard_normal((T, F)).astype(np.float32)], axis=1) if F else xyz
    off = scene.scene_offsets(sizes)
    poss = scene.initial_possibility(T, seed=5)
    if lattice:             # equal possibilities too, inside and across scenes
        poss = (np.floor(poss * np.float32(4000)) * np.float32(2.5e-4)).astype(np.float32)
    small = sizes.index(n) if n in sizes else 0    # a scene of exactly n points is among the first picked
    poss[off[small]:off[small + 1]] *= np.float32(0.0625)
    dev = _dev()
    S, Mmax = len(sizes), max(sizes)
    with torch.cuda.device(dev):
        cloud_d = torch.from_numpy(cloud).to(dev)           # F > 0: rows 3 + F floats apart
        poss_d = torch.from_numpy(poss).to(dev)
        ws = ops.scenes_workspace(dev, S, Mmax, n)
        ops.scenes_init(torch.from_numpy(off).to(dev), poss_d, ws, Mmax)
        k, seen = 0, set()
        while k < crops:
            B = min(3 if k % 4 == 3 else 1, crops - k)      # single crops and batches of three
            nz = rs.normal(0, noise, (B, 3)).astype(np.float32) if noise > 0 else None
            want = [scene.scenes_crop(xyz, off, poss, n, None if nz is None else nz[b]) for b in range(B)]
            idx = torch.full((B, n), -1, dtype=torch.int64, device=dev)
            sc = torch.full((B,), -1, dtype=torch.int64, device=dev)
            ops.scenes_crop(cloud_d, poss_d, n, idx, sc, ws, S, Mmax, None if nz is None else torch.from_numpy(nz).to(dev))
            assert sc.cpu().tolist() == [s for s, _ in want], f"crop {k}: scenes differ"
            got = idx.cpu().numpy()
            for b in range(B):
                assert np.array_equal(got[b], want[b][1]), f"crop {k + b}: indices differ"
            assert np.array_equal(poss_d.cpu().numpy().view(np.uint32), poss.view(np.uint32)), \
                f"crop {k}: possibilities differ"
            seen.update(s for s, _ in want)
            k += B
        assert small in seen and (S == 1 or len(seen) > 1)


def test_one_scene_without_noise_equals_rl_scene_crop():
    from randlanet import _ops as ops
    from randlanet.utils import scene
    dev = _dev()
    rs = np.random.RandomState(2)
    M, n = 300000, 8192
    cloud = _xyz(rs, M, lattice=True)
    with torch.cuda.device(dev):
        cloud_d = torch.from_numpy(cloud).to(dev)
        pa = torch.from_numpy(scene.initial_possibility(M, 1)).to(dev)
        pb = pa.clone()
        ws1 = ops.scene_workspace(dev, M, n)
        ws2 = ops.scenes_workspace(dev, 1, M, n)
        ops.scenes_init(torch.tensor([0, M], dtype=torch.int64, device=dev), pb, ws2, M)
        rows = torch.empty((n, 3), dtype=torch.float32, device=dev)
        i32 = torch.empty(n, dtype=torch.int32, device=dev)
        i64 = torch.empty((1, n), dtype=torch.int64, device=dev)
        sc = torch.empty(1, dtype=torch.int64, device=dev)
        for k in range(12):
            ops.scene_crop(cloud_d, pa, n, rows, i32, ws1)
            ops.scenes_crop(cloud_d, pb, n, i64, sc, ws2, 1, M)
            assert torch.equal(i32.long(), i64[0]) and int(sc.item()) == 0, f"crop {k}"
            assert torch.equal(pa.view(torch.int32), pb.view(torch.int32)), f"crop {k}"


def _close(got, want):
    """tests/test_pipeline_gpu.py's tolerance: one float32 ulp of the value (or of the extent near zero), few differ."""
    scale = max(1.0, float(np.abs(want).max()))
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.maximum(np.spacing(np.abs(want).astype(np.float32)), np.spacing(np.float32(scale))).astype(np.float64)
    return bool((diff <= ulp).all()) and float((diff > 0).mean()) < 0.05


def _scenes(rs, sizes, F):
    # float64 coordinates: the loader converts them to float32 once
    return [(rs.uniform(0, 4, (M, 3)), rs.standard_normal((M, F)).astype(np.float32), rs.randint(0, 5, M).astype(np.int64))
            for M in sizes]


@pytest.mark.parametrize("noise", [0.0, 0.3])
def test_loader_batches_match_a_host_restatement(noise):
    from randlanet.utils import scene
    from randlanet.utils.augmentation import AugmentationSettings, perturbate_point_cloud
    from randlanet.utils.scene_loader import get_scene_crop_loader
    rs = np.random.RandomState(12)
    sizes, n, B, crops = [5000, 3000, 8000], 2048, 3, 7
    scenes = _scenes(rs, sizes, 2)
    aug = AugmentationSettings()
    torch_state = torch.get_rng_state()
    np.random.seed(4)
    loader = get_scene_crop_loader(scenes, n, B, crops, center_noise=noise, augmentation_settings=aug, seed=2, device="cuda")
    assert len(loader) == 3 and loader.batch_size == B and len(loader.dataset) == crops
    got = [(i.cpu().numpy(), lab.cpu().numpy(), s.cpu().numpy()) for i, lab, s in loader]
    after = np.random.get_state()[1].copy()
    assert torch.equal(torch.get_rng_state(), torch_state)
    assert [g[0].shape[0] for g in got] == [3, 3, 1]
    # the host restatement: utils/scene.py crops, then utils/augmentation with the same numpy stream
    np.random.seed(4)
    xyz = np.concatenate([x.astype(np.float32) for x, _, _ in scenes])
    feat = np.concatenate([f for _, f, _ in scenes])
    lab = np.concatenate([l for _, _, l in scenes])
    off = scene.scene_offsets(sizes)
    poss = scene.initial_possibility(xyz.shape[0], 2)
    for inp, lb, sc in got:
        for b in range(inp.shape[0]):
            c = scene.centre_noise(noise)
            s, idx = scene.scenes_crop(xyz, off, poss, n, c if noise > 0 else None)
            want = perturbate_point_cloud(xyz[idx], aug).astype(np.float32)
            assert sc[b] == s
            assert np.array_equal(lb[b], lab[idx])
            assert np.array_equal(inp[b][:, 3:], feat[idx])
            assert _close(inp[b][:, :3], want)
    assert np.array_equal(np.random.get_state()[1], after)
    assert np.array_equal(loader.possibility.cpu().numpy().view(np.uint32), poss.view(np.uint32))


def test_next_batch_does_not_wait_for_the_gpu():
    from randlanet import _hip as H
    from randlanet.utils.augmentation import AugmentationSettings
    from randlanet.utils.scene_loader import get_scene_crop_loader
    rs = np.random.RandomState(3)
    loader = get_scene_crop_loader(_scenes(rs, [200000, 50000], 0), 4096, 4, 64, center_noise=0.1,
                                   augmentation_settings=AugmentationSettings(), device="cuda")
    it = iter(loader)
    for _ in range(6):                                  # warm-up: the staging ring, the allocator
        next(it)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    for _ in range(3):                                  # 60 ms of spin queued ahead of the next batch
        H.check(H.lib().rl_spin_us(20000, stream.cuda_stream), "rl_spin_us")
    inp, lab, sc = next(it)
    assert not stream.query(), "producing a batch waited for the GPU"
    torch.cuda.synchronize()
    assert inp.shape == (4, 4096, 3) and sc.is_cuda
    it.close()                                          # (drains the error words of the launched batches)
    assert not loader._checks


def _labelled_scene(rs, M):
    xyz = rs.uniform((0, 0, -1), (6, 6, 1), (M, 3)).astype(np.float32)
    return xyz, np.zeros((M, 0), np.float32), (xyz[:, 2] > 0).astype(np.int64)


def _train(train, val):
    from randlanet import AugmentationSettings, Model, RandLANetSettings, TrainingSettings
    torch.manual_seed(0)
    np.random.seed(0)
    model = Model(RandLANetSettings(n_classes=2, n_points=2048, n_neighbors=8, layer_sizes=[8, 16, 32, 32]))
    hist = []
    model.train_scenes(train, val, TrainingSettings(epochs=4, batch_size=4, learning_rate=1e-2, early_stopping=False),
                       AugmentationSettings(), crops_per_epoch=22, validation_crops=8, center_noise=0.05, seed=3,
                       class_names=["below", "above"], callbacks=[lambda e, m: hist.append(m["loss"])])
    return model, hist


def test_train_scenes_end_to_end():
    rs = np.random.RandomState(8)
    train = [_labelled_scene(rs, M) for M in (30000, 45000, 20000)]
    val = [_labelled_scene(rs, 25000)]
    held_out, _, truth = _labelled_scene(rs, 40000)
    m1, h1 = _train(train, val)
    m2, h2 = _train(train, val)
    for (k, a), b in zip(m1.module.state_dict().items(), m2.module.state_dict().values()):
        assert torch.equal(a, b), k
    assert h1 == h2
    assert h1[-1] < h1[0], h1
    np.random.seed(1)
    acc = float((m1.predict_scene(held_out, batch_size=4).argmax(0) == truth).mean())
    print(f"train_scenes: losses {h1}, held-out accuracy {acc:.4f}")
    assert acc > 0.7, acc
