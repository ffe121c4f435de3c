"""The scene kernels (csrc/scene.hip, rl_scene_*) against their numpy twin (utils/scene.py), and Model.predict_scene on
the MI355X against the same weights on the CPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _tie_heavy(rs: np.random.RandomState, M: int, extent: float) -> np.ndarray:
    """Coordinates on a coarse lattice (many equal distances) with a quarter of the points duplicated."""
    xyz = np.floor(rs.uniform(0, extent, (M, 3))).astype(np.float32) * np.float32(0.25)
    xyz[rs.randint(0, M, M // 4)] = xyz[rs.randint(0, M, M // 4)]
    return xyz


@pytest.mark.parametrize("M,n,F,pad", [(1000, 300, 0, 0), (1000, 1000, 2, 1), (50000, 4096, 0, 0),
                                       (50000, 4096, 3, 2), (3000000, 40960, 0, 0), (3000000, 40960, 1, 0)])
def test_scene_crop_bitwise_twin(M, n, F, pad):
    from randlanet import _ops as ops
    from randlanet.utils import scene
    dev = _dev()
    rs = np.random.RandomState(M + F)
    xyz = _tie_heavy(rs, M, extent=max(8.0, round(M ** (1 / 3))))
    cloud = np.concatenate([xyz, rs.standard_normal((M, F)).astype(np.float32)], axis=1) if F else xyz
    dim = 3 + F
    if F % 2:       # equal possibilities too: the pick must break ties by the lowest index
        poss = np.floor(scene.initial_possibility(M, seed=F) * np.float32(4000)) * np.float32(2.5e-4)
    else:
        poss = scene.initial_possibility(M, seed=F)
    poss = poss.astype(np.float32)
    with torch.cuda.device(dev):
        cloud_d = torch.from_numpy(cloud).to(dev)
        poss_d = torch.from_numpy(poss).to(dev)
        ws = ops.scene_workspace(dev, M, n)
        rows = torch.full((n, dim + pad), -7.0, dtype=torch.float32, device=dev)
        idx = torch.empty(n, dtype=torch.int32, device=dev)
        for k in range(8):
            want = scene.crop(cloud, poss, n)
            ops.scene_crop(cloud_d, poss_d, n, rows, idx, ws)
            got = idx.cpu().numpy()
            assert np.array_equal(got, want), f"crop {k}: indices differ"
            r = rows.cpu().numpy()
            assert np.array_equal(r[:, :dim].view(np.uint32), cloud[want].view(np.uint32)), f"crop {k}: rows differ"
            assert np.all(r[:, dim:] == -7.0)
            assert np.array_equal(poss_d.cpu().numpy().view(np.uint32), poss.view(np.uint32)), \
                f"crop {k}: possibilities differ"


def test_scene_accumulate_and_min_count():
    from randlanet import _ops as ops
    from randlanet.utils import scene
    dev = _dev()
    rs = np.random.RandomState(3)
    M, C, n = 20000, 13, 6000
    s, oms = scene.blend_factors(0.95)
    prob = np.zeros((M, C), np.float32)
    count = np.zeros(M, np.int32)
    crops = [np.sort(rs.choice(M, n, replace=False)).astype(np.int32) for _ in range(3)]
    crops[1] = np.union1d(crops[0][: n // 2], crops[1])[:n].astype(np.int32)   # overlaps the first crop
    logits = [(3 * rs.standard_normal((C, n))).astype(np.float32) for _ in crops]
    with torch.cuda.device(dev):
        prob_d = torch.zeros((M, C), dtype=torch.float32, device=dev)
        count_d = torch.zeros(M, dtype=torch.int32, device=dev)
        ws = ops.scene_workspace(dev, M, n)
        low = torch.full((1,), -1, dtype=torch.int32, device=dev)
        for idx, lg in zip(crops, logits):
            scene.accumulate(prob, count, lg, idx, oms, s)
            ops.scene_accumulate(torch.from_numpy(lg).to(dev), torch.from_numpy(idx).to(dev), float(oms), float(s),
                                 prob_d, count_d)
        ops.scene_min_count(count_d, low, ws)
        assert np.array_equal(count_d.cpu().numpy(), count)
        got = prob_d.cpu().numpy()
        assert np.all(np.abs(got - prob) <= 1e-6 * np.abs(prob) + 1e-12)
        assert int(low.item()) == int(count.min()) == 0
        count_d += 2
        count_d[12345] = 1
        ops.scene_min_count(count_d, low, ws)
        assert int(low.item()) == 1


def _models(n_points, seed=0):
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(seed)
    st = RandLANetSettings(n_classes=6, n_points=n_points, n_neighbors=8, layer_sizes=[16, 32])
    gpu = Model(st, use_gpu=True)
    assert gpu.device.type == "cuda"
    weights = {k: v.detach().cpu().clone() for k, v in gpu.module.state_dict().items()}
    cpu = Model(RandLANetSettings(**vars(st)), weights=weights, use_gpu=False)
    return gpu, cpu


def test_predict_scene_gpu_matches_cpu_model():
    gpu, cpu = _models(8192)
    rs = np.random.RandomState(9)
    xyz = np.concatenate([rs.uniform(0, 30, (150000, 3)), rs.uniform(0, 5, (50000, 3))]).astype(np.float32)
    np.random.seed(21)
    out_g, cnt_g = gpu.predict_scene(xyz, votes=2, batch_size=4, seed=1, return_counts=True)
    state_g = np.random.get_state()[1].copy()
    np.random.seed(21)
    out_c, cnt_c = cpu.predict_scene(xyz, votes=2, batch_size=4, seed=1, return_counts=True)
    assert np.array_equal(np.random.get_state()[1], state_g)
    assert np.array_equal(cnt_g, cnt_c), "different crop sequences"
    assert cnt_g.min() >= 2
    assert np.abs(out_g - out_c).max() < 1e-4
    top = np.sort(out_c, axis=0)
    clear = (top[-1] - top[-2]) > 1e-4
    assert np.array_equal(out_g.argmax(0)[clear], out_c.argmax(0)[clear])


def test_predict_scene_gpu_small_scene_equals_predict():
    gpu, _ = _models(4096, seed=1)
    xyz = np.random.RandomState(4).uniform(0, 10, (3000, 3)).astype(np.float32)
    np.random.seed(6)
    ref = gpu.predict(xyz, prepostprocess=False)
    np.random.seed(6)
    out = gpu.predict_scene(xyz)
    assert np.abs(out - ref).max() < 1e-6
