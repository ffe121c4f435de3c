"""Grid subsampling and whole-scene evaluation on the MI355X: csrc/grid.hip against the numpy twin (utils/grid.py), bit for
bit; rl_scene_confusion against the twin's table; Model.predict_scene(grid=) / evaluate_scenes on a GPU-placed model against
the CPU-placed one; Model.train_scenes(grid=)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F32 = np.float32


def _dev():
    return torch.device("cuda", 0)


# --------------------------------------------------------------------------------------------------- inputs
def _uniform_negative(rs, M):
    return rs.uniform(-7, 5, (M, 3)).astype(F32), 0.205


def _face_lattice(rs, M, half=12, cell=0.3):
    """Points exactly on cell faces: integer multiples of float32(cell), computed in float32, around zero."""
    return rs.randint(-half, half + 1, (M, 3)).astype(F32) * F32(cell), cell


def _one_cell(rs, M):
    return rs.uniform(0.31, 0.59, (M, 3)).astype(F32), 0.3


def _lonely(rs, M):
    """Every point in a cell of its own: M distinct nodes of a 40^3 lattice, at the cell centres."""
    nodes = rs.permutation(40 ** 3)[:M]
    k = np.stack([nodes % 40, (nodes // 40) % 40, nodes // 1600], axis=1).astype(F32)
    return ((k - F32(20) + F32(0.5)) * F32(0.25)).astype(F32), 0.25


def _flat(rs, M):
    x = rs.uniform(-20, 20, (M, 3)).astype(F32)
    x[:, 2] = F32(1.25)
    return x, 0.5


def _wide(rs, M):
    """A small cell over a wide extent: about 2*10^6 cells per axis, a key of more than 32 bits."""
    return rs.uniform(0, 2000, (M, 3)).astype(F32), 0.001


# name: (generator, M, F, n_classes or 0)
CASES = {
    "single": (_uniform_negative, 1, 0, 0),
    "single_full": (_uniform_negative, 1, 3, 13),
    "uniform_1000": (_uniform_negative, 1000, 3, 13),
    "uniform_1000_xyz": (_uniform_negative, 1000, 0, 0),
    "lattice_50000": (_face_lattice, 50000, 0, 0),
    "lattice_50000_full": (_face_lattice, 50000, 3, 13),
    "one_cell_50000": (_one_cell, 50000, 2, 13),
    "lonely_1000": (_lonely, 1000, 0, 5),
    "lonely_50000": (_lonely, 50000, 3, 0),
    "flat_50000": (_flat, 50000, 1, 4),
    "wide_key_50000": (_wide, 50000, 0, 3),
    "uniform_2e6_full": (_uniform_negative, 2_000_000, 3, 13),
    "lattice_2e6_xyz": (lambda rs, M: _face_lattice(rs, M, half=40), 2_000_000, 0, 0),
}


def _inputs(case):
    gen, M, F, C = CASES[case]
    rs = np.random.RandomState(sum(map(ord, case)))
    xyz, cell = gen(rs, M)
    feats = rs.standard_normal((M, F)).astype(F32) if F else None
    labels = rs.randint(0, C, M) if C else None
    return xyz, feats, labels, cell, (C or None)


def _assert_same(res, ref):
    for name, a, b in zip(("xyz", "features", "labels", "inverse", "count"), res, ref):
        if b is None:
            assert a is None, name
            continue
        assert a is not None and a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), f"{name}: {int((a != b).sum())} entries differ"


@pytest.mark.parametrize("case", list(CASES))
def test_grid_subsample_bitwise_twin(case):
    from randlanet.utils import grid
    xyz, feats, labels, cell, C = _inputs(case)
    ref = grid.grid_subsample_host(xyz, feats, labels, cell=cell, n_classes=C)
    res = grid.grid_subsample(xyz, feats, labels, cell=cell, n_classes=C, device=_dev())
    _assert_same(res, ref)
    M, V = xyz.shape[0], ref.xyz.shape[0]
    if case.startswith("one_cell"):
        assert V == 1
    if case.startswith("lonely"):
        assert V == M
    c = F32(cell)
    o, dims = grid.grid_geometry(xyz, c)
    if case.startswith("flat"):
        assert dims[2] == 1
    if case.startswith("wide"):
        assert grid.key_bits(dims) > 32


def test_grid_subsample_default_device_is_the_gpu_and_deterministic():
    from randlanet import _hip
    from randlanet.utils import grid
    xyz, feats, labels, cell, C = _inputs("uniform_2e6_full")
    a = grid.grid_subsample(xyz, feats, labels, cell=cell, n_classes=C)          # device=None: a GPU is available
    assert _hip.lib().rl_last_kernel() == b"grid_reduce"
    b = grid.grid_subsample(xyz, feats, labels, cell=cell, n_classes=C, device="cuda")
    _assert_same(a, b)


def test_device_tensors_and_read_backs():
    from randlanet import _ops as ops
    from randlanet.utils import grid
    dev = _dev()
    xyz, feats, labels, cell, C = _inputs("uniform_1000")
    cloud = np.concatenate((xyz, feats), axis=1)
    with torch.cuda.device(dev):
        rows, lab, inverse, count = ops.grid_subsample(torch.from_numpy(cloud).to(dev), torch.from_numpy(labels).to(dev),
                                                       cell, C)
    assert rows.is_cuda and lab.is_cuda and inverse.is_cuda and count.is_cuda
    ref = grid.grid_subsample_host(xyz, feats, labels, cell=cell, n_classes=C)
    assert np.array_equal(rows.cpu().numpy(), np.concatenate((ref.xyz, ref.features), axis=1))
    assert np.array_equal(lab.cpu().numpy(), ref.labels) and np.array_equal(inverse.cpu().numpy(), ref.inverse)
    assert np.array_equal(count.cpu().numpy(), ref.count)


def test_too_fine_a_grid_is_refused_from_the_device_dims():
    from randlanet.utils import grid
    xyz = np.array([[0, 0, 0], [3000, 0, 0], [1, 2, 3]], F32)
    with pytest.raises(ValueError, match="2\\^21"):
        grid.grid_subsample(xyz, cell=0.001, device=_dev())


# ----------------------------------------------------------------------------------------------- rl_scene_confusion
@pytest.mark.parametrize("C", [6, 70])
def test_scene_confusion_equals_the_twin(C):
    from randlanet import _ops as ops
    from randlanet.utils import grid
    dev = _dev()
    rs = np.random.RandomState(C)
    V, M = 5000, 200_000
    prob = (rs.randint(0, 4, (V, C)) / 4).astype(F32)             # quantised: many ties for the argmax
    prob[::7] = rs.uniform(0, 1, prob[::7].shape).astype(F32)
    labels = rs.randint(-1, C + 1, M).astype(np.int64)            # -1 and C: unlabelled, skipped
    inverse = rs.randint(0, V, M).astype(np.int32)
    with torch.cuda.device(dev):
        prob_d, lab_d, inv_d = (torch.from_numpy(a).to(dev) for a in (prob, labels, inverse))
        table = torch.zeros((C, C), dtype=torch.int64, device=dev)
        ops.scene_confusion(prob_d, lab_d, table, inv_d)
        want = grid.confusion(prob_d.cpu().numpy(), labels, C, inverse)
        assert np.array_equal(table.cpu().numpy(), want)
        assert int(want.sum()) == int(((labels >= 0) & (labels < C)).sum())
        # without inverse: a point reads its own row
        table0 = torch.zeros((C, C), dtype=torch.int64, device=dev)
        ops.scene_confusion(prob_d, lab_d[:V].contiguous(), table0)
        want0 = grid.confusion(prob, labels[:V], C)
        assert np.array_equal(table0.cpu().numpy(), want0)
        # a second call accumulates
        ops.scene_confusion(prob_d, lab_d[:V].contiguous(), table)
        assert np.array_equal(table.cpu().numpy(), want + want0)


# --------------------------------------------------------------------------------------------------------- Model
def _models(n_points, n_classes=6, seed=0):
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(seed)
    st = RandLANetSettings(n_classes=n_classes, n_points=n_points, n_neighbors=8, layer_sizes=[16, 32])
    gpu = Model(st, use_gpu=True)
    assert gpu.device.type == "cuda"
    weights = {k: v.detach().cpu().clone() for k, v in gpu.module.state_dict().items()}
    cpu = Model(RandLANetSettings(**vars(st)), weights=weights, use_gpu=False)
    return gpu, cpu


def test_predict_scene_grid_gpu_matches_cpu_model():
    """The bounds are those of tests/test_scene_gpu.py::test_predict_scene_gpu_matches_cpu_model."""
    from randlanet.utils import grid
    gpu, cpu = _models(8192)
    rs = np.random.RandomState(9)
    xyz = np.concatenate([rs.uniform(0, 30, (150000, 3)), rs.uniform(0, 5, (50000, 3))]).astype(F32)
    cell = 0.8
    V = grid.grid_subsample_host(xyz, cell=cell).xyz.shape[0]
    assert 8192 < V < xyz.shape[0] // 2
    np.random.seed(21)
    out_g, cnt_g = gpu.predict_scene(xyz, votes=2, batch_size=4, seed=1, return_counts=True, grid=cell)
    state_g = np.random.get_state()[1].copy()
    np.random.seed(21)
    out_c, cnt_c = cpu.predict_scene(xyz, votes=2, batch_size=4, seed=1, return_counts=True, grid=cell)
    assert np.array_equal(np.random.get_state()[1], state_g)
    assert out_g.shape == out_c.shape == (6, xyz.shape[0])
    assert np.array_equal(cnt_g, cnt_c), "different crop sequences"
    assert cnt_g.min() >= 2
    assert np.abs(out_g - out_c).max() < 1e-4
    top = np.sort(out_c, axis=0)
    clear = (top[-1] - top[-2]) > 1e-4
    assert np.array_equal(out_g.argmax(0)[clear], out_c.argmax(0)[clear])


def _eval_scenes(C):
    scenes = []
    for k, M in enumerate((60000, 40000)):
        rs = np.random.RandomState(30 + k)
        xyz = rs.uniform((0, 0, 0), (16, 16, 4), (M, 3)).astype(F32)
        labels = (np.floor(xyz[:, 0] / 4) + 2 * np.floor(xyz[:, 2] / 2)).astype(np.int64) % C
        labels[rs.randint(0, M, M // 20)] = -1                    # unlabelled points
        scenes.append((xyz, None, labels))
    return scenes


@pytest.mark.parametrize("cell", [0.4, None])
def test_evaluate_scenes_gpu_matches_cpu_model(cell):
    """sum |conf_gpu - conf_cpu| <= 2u, u = the raw points whose top-two margin on the CPU side is <= 1e-4 (the margin above
    which test_predict_scene_gpu_matches_cpu_model requires equal argmax): each such point moves at most one count out of one
    entry and into another.  u must stay under 1 % of the points for the bound to say something."""
    C = 6
    gpu, cpu = _models(4096, n_classes=C, seed=2)
    scenes = _eval_scenes(C)
    names = [f"k{c}" for c in range(C)]
    kw = dict(grid=cell, votes=1, batch_size=4, seed=3)
    np.random.seed(8)
    got, conf_g = gpu.evaluate_scenes(scenes, names, return_confusion=True, **kw)
    state_g = np.random.get_state()[1].copy()
    np.random.seed(8)
    want, conf_c = cpu.evaluate_scenes(scenes, names, return_confusion=True, **kw)
    assert np.array_equal(np.random.get_state()[1], state_g)
    np.random.seed(8)
    u = 0
    for xyz, feats, _ in scenes:
        out = cpu.predict_scene(xyz, feats, **kw)
        top = np.sort(out, axis=0)
        u += int(((top[-1] - top[-2]) <= 1e-4).sum())
    total = sum(s[0].shape[0] for s in scenes)
    labelled = sum(int((s[2] >= 0).sum()) for s in scenes)
    diff = int(np.abs(conf_g - conf_c).sum())
    print(f"evaluate_scenes cell={cell}: u={u} of {total} points, sum|conf_gpu - conf_cpu|={diff}")
    assert u < 0.01 * total
    assert conf_g.dtype == np.int64 and int(conf_g.sum()) == int(conf_c.sum()) == labelled
    assert diff <= 2 * u
    assert list(got) == list(want) == ["OA", "mAcc", "mIoU"] + [f"{n} IoU" for n in names]
    # every class is labelled somewhere and the table has off-diagonal mass: the comparison is not between empty tables
    assert (conf_c.sum(axis=1) > 0).all() and (conf_c > 0).sum() >= C


def test_train_scenes_with_grid(monkeypatch):
    from randlanet import AugmentationSettings, Model, RandLANetSettings, TrainingSettings
    from randlanet import model as model_module
    from randlanet.utils import grid
    rs = np.random.RandomState(5)

    def labelled(M):
        xyz = rs.uniform((0, 0, -1), (6, 6, 1), (M, 3)).astype(F32)
        return xyz, rs.standard_normal((M, 2)).astype(F32), (xyz[:, 2] > 0).astype(np.int64) + (xyz[:, 0] > 3)

    train, val = [labelled(30000), labelled(40000)], [labelled(25000)]
    cell, C = 0.2, 3
    loaders = []
    make = model_module.get_scene_crop_loader

    def recording(*a, **k):
        loaders.append(make(*a, **k))
        return loaders[-1]

    monkeypatch.setattr(model_module, "get_scene_crop_loader", recording)
    torch.manual_seed(0)
    np.random.seed(0)
    model = Model(RandLANetSettings(n_classes=C, n_points=2048, n_features=2, n_neighbors=8, layer_sizes=[8, 16, 32, 32]))
    seen = []
    model.train_scenes(train, val, TrainingSettings(epochs=1, batch_size=2, learning_rate=1e-2, early_stopping=False),
                       AugmentationSettings(), crops_per_epoch=4, validation_crops=2, seed=3, class_names=["a", "b", "c"],
                       callbacks=[lambda e, m: seen.append(m["loss"])], grid=cell)
    assert len(seen) == 1 and np.isfinite(seen[0])
    assert len(loaders) == 2
    for loader, scenes in zip(loaders, (train, val)):
        subs = [grid.grid_subsample_host(x, f, l, cell=cell, n_classes=C) for x, f, l in scenes]
        sizes = [s.xyz.shape[0] for s in subs]
        assert all(2048 <= v < x.shape[0] for v, (x, _, _) in zip(sizes, scenes))
        assert np.array_equal(np.diff(loader._off.cpu().numpy()), sizes)
        assert np.array_equal(loader._lab.cpu().numpy(), np.concatenate([s.labels for s in subs]))
        assert np.array_equal(loader._xyz.cpu().numpy(), np.concatenate([s.xyz for s in subs]))
        assert np.array_equal(loader._feat.cpu().numpy(), np.concatenate([s.features for s in subs]))
    # a scene that falls below n_points after subsampling: check_scenes' error
    with pytest.raises(ValueError, match="fewer than the crop size n=2048"):
        model.train_scenes([labelled(3000)], val, TrainingSettings(epochs=1, batch_size=2), crops_per_epoch=2,
                           validation_crops=2, class_names=["a", "b", "c"], grid=1.0)
