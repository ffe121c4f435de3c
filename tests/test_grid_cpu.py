"""Grid subsampling and whole-scene evaluation without a GPU: the numpy twin (utils/grid.py) against a plain-Python dict
restatement, its properties and refusals, the confusion matrix and its metrics, the CPU-placed Model (predict_scene(grid=),
evaluate_scenes, train_scenes(grid=)) and the host-side argument checks of the rl_grid_* / rl_scene_confusion entry points."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# --------------------------------------------------------------------------------------------------- inputs
def uniform_negative(M, seed=0):
    rs = np.random.RandomState(seed)
    return rs.uniform(-7, 5, (M, 3)).astype(F32)


def face_lattice(M, cell, seed=0):
    """Points exactly on cell faces: integer multiples of float32(cell), computed in float32, around zero."""
    rs = np.random.RandomState(seed)
    k = rs.randint(-12, 13, (M, 3)).astype(F32)
    return k * F32(cell)


def _extras(M, F, C, seed):
    rs = np.random.RandomState(seed + 100)
    feats = rs.standard_normal((M, F)).astype(F32) if F else None
    labels = rs.randint(0, C, M) if C else None
    return feats, labels


# ------------------------------------------------------------------------------------- the independent restatement
def restate(xyz, features, labels, cell, n_classes):
    """Cells as tuples in a dict, sorted by (z, y, x); sequential float64 sums in point order; plain Python."""
    x = np.asarray(xyz).astype(F32)
    M = x.shape[0]
    c = F32(cell)
    cloud = x if features is None else np.concatenate((x, np.asarray(features).astype(F32)), axis=1)
    o = []
    for a in range(3):
        lo = F32(min(x[:, a]))
        q = F32(lo / c)
        o.append(F32(F32(np.floor(q)) * c))
    cells = {}
    for i in range(M):
        v = []
        for a in range(3):
            d = F32(x[i, a] - o[a])
            q = F32(d / c)
            v.append(max(int(np.floor(q)), 0))
        cells.setdefault((v[2], v[1], v[0]), []).append(i)
    order = sorted(cells)
    V, dim = len(order), cloud.shape[1]
    out = np.empty((V, dim), F32)
    inverse = np.empty(M, np.int32)
    count = np.empty(V, np.int32)
    lab = np.empty(V, np.int64) if labels is not None else None
    for r, cellid in enumerate(order):
        members = cells[cellid]                      # ascending point index by construction
        count[r] = len(members)
        for k in range(dim):
            s = 0.0
            for i in members:
                s += float(cloud[i, k])
            out[r, k] = F32(s / len(members))
        for i in members:
            inverse[i] = r
        if labels is not None:
            h = [0] * n_classes
            for i in members:
                h[int(labels[i])] += 1
            lab[r] = h.index(max(h))
    return out[:, :3], (out[:, 3:] if features is not None else None), lab, inverse, count


def assert_same(res, ref):
    names = ("xyz", "features", "labels", "inverse", "count")
    for name, a, b in zip(names, res, ref):
        if b is None:
            assert a is None, name
            continue
        assert a is not None and a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), name


CASES = {
    "uniform_negative": lambda: (uniform_negative(20000, 1), 0.3),
    "face_lattice": lambda: (face_lattice(20000, 0.3, 2), 0.3),
    "face_lattice_pow2": lambda: (face_lattice(5000, 0.25, 3), 0.25),
    "single_point": lambda: (np.array([[-1.7, 2.9, 0.05]], F32), 0.3),
    "one_cell": lambda: (np.random.RandomState(4).uniform(0.31, 0.59, (6000, 3)).astype(F32), 0.3),
}


@pytest.mark.parametrize("extras", ["none", "features+labels", "features", "labels"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_twin_equals_the_dict_restatement(case, extras):
    from randlanet.utils import grid
    xyz, cell = CASES[case]()
    M = xyz.shape[0]
    feats, labels = _extras(M, 3 if "features" in extras else 0, 13 if "labels" in extras else 0, M)
    C = 13 if labels is not None else None
    res = grid.grid_subsample_host(xyz, feats, labels, cell=cell, n_classes=C)
    assert_same(res, restate(xyz, feats, labels, cell, C))
    assert res.xyz.dtype == F32 and res.inverse.dtype == np.int32 and res.count.dtype == np.int32
    if case == "single_point":
        assert res.count.tolist() == [1] and np.array_equal(res.xyz, xyz)
    if case == "one_cell":
        assert res.count.tolist() == [M]


def test_float64_input_is_converted_to_float32_first():
    from randlanet.utils import grid
    xyz = np.random.RandomState(5).uniform(-3, 3, (3000, 3))
    a = grid.grid_subsample_host(xyz, cell=0.25)
    b = grid.grid_subsample_host(xyz.astype(F32), cell=0.25)
    assert_same(a, b)


# ----------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("case", ["uniform_negative", "face_lattice"])
def test_twin_properties(case):
    from randlanet.utils import grid
    xyz, cell = CASES[case]()
    M = xyz.shape[0]
    labels = np.random.RandomState(6).randint(0, 5, M)
    res = grid.grid_subsample_host(xyz, None, labels, cell=cell, n_classes=5)
    V = res.xyz.shape[0]
    assert int(res.count.sum()) == M and res.count.min() >= 1
    assert res.inverse.min() == 0 and res.inverse.max() == V - 1
    assert np.array_equal(np.unique(res.inverse), np.arange(V))
    assert np.array_equal(np.bincount(res.inverse, minlength=V), res.count)
    # the key of every output row (shared by all its points), strictly ascending
    c = F32(cell)
    o, dims = grid.grid_geometry(xyz, c)
    key = grid.cell_keys(xyz, o, dims, c)
    row_key = np.full(V, -1, np.int64)
    row_key[res.inverse] = key
    assert np.array_equal(row_key[res.inverse], key)
    assert np.all(np.diff(row_key) > 0)
    # a representative lies within one cell edge of its points on every axis (plus float32 rounding of the coordinates)
    ulp = float(np.spacing(np.abs(xyz).max()))
    assert np.abs(res.xyz[res.inverse] - xyz).max() <= cell + 4 * ulp


def test_label_ties_go_to_the_lowest_class():
    from randlanet.utils import grid
    xyz = np.array([[0.1, 0.1, 0.1]] * 4 + [[0.9, 0.1, 0.1]] * 3, F32)
    labels = np.array([3, 1, 3, 1, 2, 2, 0])
    res = grid.grid_subsample_host(xyz, None, labels, cell=0.5, n_classes=4)
    assert res.count.tolist() == [4, 3] and res.labels.tolist() == [1, 2] and res.labels.dtype == np.int64


def test_shuffled_input_gives_the_same_cells():
    from randlanet.utils import grid
    xyz, cell = CASES["uniform_negative"]()
    M = xyz.shape[0]
    labels = np.random.RandomState(7).randint(0, 6, M)
    perm = np.random.RandomState(8).permutation(M)
    a = grid.grid_subsample_host(xyz, None, labels, cell=cell, n_classes=6)
    b = grid.grid_subsample_host(xyz[perm], None, labels[perm], cell=cell, n_classes=6)
    inv_b = np.empty(M, np.int32)
    inv_b[perm] = b.inverse                          # un-shuffled: the row of original point i
    assert np.array_equal(inv_b, a.inverse)          # same occupied cells, in the same (key) order
    assert np.array_equal(a.count, b.count) and np.array_equal(a.labels, b.labels)


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from randlanet.utils import grid
    xyz = uniform_negative(100)
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cell"):
            grid.grid_subsample_host(xyz, cell=cell)
    for bad in (np.nan, np.inf, -np.inf):
        x = xyz.copy()
        x[17, 1] = bad
        with pytest.raises(ValueError, match="non-finite.*point 17"):
            grid.grid_subsample_host(x, cell=0.3)
    with pytest.raises(ValueError, match="M=0"):
        grid.grid_subsample_host(np.zeros((0, 3), F32), cell=0.3)
    with pytest.raises(ValueError, match="2\\^21"):
        grid.grid_subsample_host(np.array([[0, 0, 0], [3000, 0, 0]], F32), cell=0.001)
    labels = np.zeros(100, np.int64)
    with pytest.raises(ValueError, match="without n_classes"):
        grid.grid_subsample_host(xyz, None, labels, cell=0.3)
    for bad in (-1, 4):
        lab = labels.copy()
        lab[5] = bad
        with pytest.raises(ValueError, match=f"label {bad} of point 5"):
            grid.grid_subsample_host(xyz, None, lab, cell=0.3, n_classes=4)
    # the public function refuses the same way, on the host, whichever device it would run on
    with pytest.raises(ValueError, match="cell"):
        grid.grid_subsample(xyz, cell=0.0, device="cpu")
    with pytest.raises(ValueError, match="non-finite"):
        x = xyz.copy()
        x[0, 0] = np.nan
        grid.grid_subsample(x, cell=0.3)


def test_too_many_points_is_refused_before_any_copy():
    from randlanet.utils import grid

    class Huge:                                      # only its shape is looked at
        shape = (2 ** 31 - 1, 3)

    with pytest.raises(ValueError, match="M=2147483647"):
        grid.grid_subsample_host(Huge(), cell=0.3)


def test_public_function_on_the_cpu_is_the_twin():
    from randlanet.utils import grid
    xyz, cell = CASES["uniform_negative"]()
    feats, labels = _extras(xyz.shape[0], 2, 4, 9)
    assert_same(grid.grid_subsample(xyz, feats, labels, cell=cell, n_classes=4, device="cpu"),
                grid.grid_subsample_host(xyz, feats, labels, cell=cell, n_classes=4))


# -------------------------------------------------------------------------------------- confusion and its metrics
def test_confusion_by_hand():
    from randlanet.utils import grid
    prob = np.array([[0.5, 0.5, 0.0],      # tie -> class 0
                     [0.1, 0.7, 0.2],
                     [0.0, 0.2, 0.2],      # tie -> class 1
                     [0.3, 0.3, 0.3]], F32)  # tie -> class 0
    labels = np.array([0, 1, 2, 0, -1, 3, 1])
    inverse = np.array([0, 1, 2, 3, 1, 1, 0], np.int32)
    conf = grid.confusion(prob, labels, 3, inverse)
    assert conf.dtype == np.int64
    assert conf.tolist() == [[2, 0, 0], [1, 1, 0], [0, 1, 0]]
    # without inverse every point reads its own row; labels outside [0, C) are skipped
    conf2 = grid.confusion(prob, np.array([0, 1, 7, -5]), 3)
    assert conf2.tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 0]]


def test_metrics_from_confusion_use_the_pinned_conventions():
    from randlanet.utils import grid, metrics
    # class 2 absent from the labels but predicted; class 3 neither labelled nor predicted (empty union)
    conf = np.array([[5, 1, 1, 0],
                     [2, 7, 0, 0],
                     [0, 0, 0, 0],
                     [0, 0, 0, 0]], np.int64)
    cnt = np.stack([np.diag(conf), conf.sum(1), conf.sum(0)]).astype(np.float64)
    oa, acc = metrics.accuracy_from_counts(cnt)
    miou, ious = metrics.iou_from_counts(cnt)
    d = grid.metrics_from_confusion(conf)
    assert list(d) == ["OA", "mAcc", "mIoU", "class 0 IoU", "class 1 IoU", "class 2 IoU", "class 3 IoU"]
    assert "loss" not in d
    assert d["OA"] == oa == float(F32(12) / F32(16))
    assert d["mAcc"] == float(np.mean(acc)) and acc[2] == 1.0 and acc[3] == 1.0
    assert d["mIoU"] == miou and [d[f"class {c} IoU"] for c in range(4)] == ious
    assert ious[2] == 0.0 and ious[3] == 1.0 and ious[0] == float(F32(5) / F32(9))
    named = grid.metrics_from_confusion(conf, ["a", "b", "c", "d"])
    assert list(named)[3:] == ["a IoU", "b IoU", "c IoU", "d IoU"] and named["b IoU"] == ious[1]


# ------------------------------------------------------------------------------------------- CPU-placed model
def _model(n_points=2048, n_classes=5, n_features=0, seed=0):
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(seed)
    return Model(RandLANetSettings(n_classes=n_classes, n_points=n_points, n_features=n_features, n_neighbors=8,
                                   layer_sizes=[16, 32]), use_gpu=False)


@pytest.fixture(scope="module")
def cpu_model():
    return _model()


def test_predict_scene_grid_projects_the_sub_cloud(cpu_model):
    from randlanet.utils import grid
    xyz = np.random.RandomState(0).uniform(0, 16, (20000, 3)).astype(F32)
    cell = 1.0
    sub = grid.grid_subsample_host(xyz, cell=cell)
    V = sub.xyz.shape[0]
    assert cpu_model.settings.n_points < V < xyz.shape[0]
    np.random.seed(3)
    out, counts = cpu_model.predict_scene(xyz, grid=cell, batch_size=2, return_counts=True)
    C = cpu_model.settings.n_classes
    assert out.shape == (C, xyz.shape[0]) and out.dtype == F32
    assert np.abs(out.sum(axis=0) - 1).max() < 1e-5
    np.random.seed(3)
    ref, ref_counts = cpu_model.predict_scene(sub.xyz, batch_size=2, return_counts=True)
    assert np.array_equal(out, ref[:, sub.inverse]) and np.array_equal(counts, ref_counts[sub.inverse])
    # constant within a cell
    first = np.full(V, -1, np.int64)
    first[sub.inverse[::-1]] = np.arange(xyz.shape[0])[::-1]
    assert np.array_equal(out, out[:, first[sub.inverse]])


def test_predict_scene_grid_with_lonely_points_is_predict_scene(cpu_model):
    from randlanet.utils import grid
    xyz = np.random.RandomState(1).uniform(0, 20, (3000, 3)).astype(F32)
    cell = 1e-3
    sub = grid.grid_subsample_host(xyz, cell=cell)
    assert sub.xyz.shape[0] == xyz.shape[0]                       # every point alone in its cell
    order = np.argsort(sub.inverse)
    assert np.array_equal(sub.xyz, xyz[order])
    np.random.seed(4)
    out = cpu_model.predict_scene(xyz, grid=cell, batch_size=2)
    np.random.seed(4)
    ref = cpu_model.predict_scene(xyz[order], batch_size=2)
    assert np.abs(out - ref[:, sub.inverse]).max() <= 1e-6


def test_predict_scene_grid_with_features():
    m = _model(n_features=2, n_classes=3)
    rs = np.random.RandomState(2)
    xyz = rs.uniform(0, 12, (9000, 3)).astype(F32)
    feats = rs.standard_normal((9000, 2)).astype(F32)
    np.random.seed(0)
    out = m.predict_scene(xyz, feats, grid=0.8, batch_size=2)
    assert out.shape == (3, 9000) and np.abs(out.sum(axis=0) - 1).max() < 1e-5


@pytest.mark.parametrize("cell", [None, 1.0])
def test_evaluate_scenes_equals_metrics_of_predict_scene(cpu_model, cell):
    from randlanet.utils import grid, metrics
    C = cpu_model.settings.n_classes
    scenes = []
    for k, M in enumerate((9000, 5000)):
        rs = np.random.RandomState(10 + k)
        xyz = rs.uniform(0, 14, (M, 3)).astype(F32)
        labels = rs.randint(0, C, M)
        labels[rs.randint(0, M, M // 10)] = -1                    # unlabelled points
        scenes.append((xyz, None, labels))
    np.random.seed(5)
    conf = np.zeros((C, C), np.int64)
    for xyz, _, labels in scenes:
        pred = cpu_model.predict_scene(xyz, grid=cell, batch_size=2).argmax(0)
        for l, p in zip(labels, pred):
            if l >= 0:
                conf[l, p] += 1
    np.random.seed(5)
    names = [f"k{c}" for c in range(C)]
    got, got_conf = cpu_model.evaluate_scenes(scenes, names, grid=cell, batch_size=2, return_confusion=True)
    assert got_conf.dtype == np.int64 and np.array_equal(got_conf, conf)
    assert int(conf.sum()) == sum(int((l >= 0).sum()) for _, _, l in scenes)
    cnt = np.stack([np.diag(conf), conf.sum(1), conf.sum(0)]).astype(np.float64)
    oa, acc = metrics.accuracy_from_counts(cnt)
    miou, ious = metrics.iou_from_counts(cnt)
    assert list(got) == ["OA", "mAcc", "mIoU"] + [f"{n} IoU" for n in names]
    assert got["OA"] == oa and got["mAcc"] == float(np.mean(acc)) and got["mIoU"] == miou
    assert [got[f"{n} IoU"] for n in names] == ious
    np.random.seed(5)
    assert cpu_model.evaluate_scenes(scenes, names, grid=cell, batch_size=2) == got
    assert got == grid.metrics_from_confusion(conf, names)


def test_train_scenes_with_grid_on_a_cpu_model_still_raises(cpu_model):
    from randlanet._hip import HipKernelError
    xyz = np.random.RandomState(0).uniform(0, 10, (4000, 3)).astype(F32)
    sc = [(xyz, np.zeros((4000, 0), F32), np.zeros(4000, np.int64))]
    with pytest.raises(HipKernelError, match="train_scenes trains on the GPU"):
        cpu_model.train_scenes(sc, sc, crops_per_epoch=2, validation_crops=2, class_names=list("abcde"), grid=0.5)


# --------------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def lib():
    from randlanet import _hip
    if not os.path.exists(_hip.library_path()):
        subprocess.check_call(["make", "-C", os.path.join(REPO, "3d_recognizer_amd", "csrc"), "-j4"])
    return _hip.lib()


GRID_SYMBOLS = ("rl_grid_workspace_bytes", "rl_grid_bounds", "rl_grid_sort", "rl_grid_heads", "rl_grid_reduce",
                "rl_scene_confusion")


def test_grid_symbols_are_exported(lib):
    from randlanet import _hip
    raw = ctypes.CDLL(_hip.library_path())
    for name in GRID_SYMBOLS:
        assert name in _hip.EXPORTS and hasattr(raw, name)
    assert lib.rl_version() == _hip.ABI_VERSION


def test_grid_argument_errors_on_the_host(lib):
    from randlanet import _hip
    M, dim = 1000, 6
    need = lib.rl_grid_workspace_bytes(M, dim)
    # two (key, index) buffers, the segment starts
    assert need >= 2 * (8 + 4) * M + 4 * (M + 1) and need % 256 == 0
    assert lib.rl_grid_workspace_bytes(0, 3) == 0 and lib.rl_grid_workspace_bytes(2 ** 31 - 1, 3) == 0
    fake = 1 << 20              # never dereferenced: every call below is refused before a launch
    E = _hip.ERR_ARGS
    # bounds
    for cell in (0.0, -0.5, float("nan"), float("inf")):
        assert lib.rl_grid_bounds(fake, M, dim, cell, fake, fake, need, None) == E
        assert b"cell" in lib.rl_last_error()
    assert lib.rl_grid_bounds(fake, 0, dim, 0.3, fake, fake, need, None) == E
    assert b"M=0" in lib.rl_last_error()
    assert lib.rl_grid_bounds(fake, 2 ** 31 - 1, dim, 0.3, fake, fake, need, None) == E
    assert lib.rl_grid_bounds(fake, M, 2, 0.3, fake, fake, need, None) == E
    assert b"dim=2" in lib.rl_last_error()
    assert lib.rl_grid_bounds(fake, M, dim, 0.3, fake, fake, need - 1, None) == E
    assert b"workspace" in lib.rl_last_error()
    assert lib.rl_grid_bounds(fake, M, dim, 0.3, fake, fake + 64, need, None) == E
    assert b"aligned" in lib.rl_last_error()
    assert lib.rl_grid_bounds(None, M, dim, 0.3, fake, fake, need, None) == E
    assert lib.rl_grid_bounds(fake, M, dim, 0.3, None, fake, need, None) == E
    assert lib.rl_grid_bounds(fake, M, dim, 0.3, fake, None, need, None) == E
    # sort
    for bits in (0, 64, -3):
        assert lib.rl_grid_sort(fake, M, dim, bits, fake, need, None) == E
        assert b"key_bits" in lib.rl_last_error()
    assert lib.rl_grid_sort(fake, M, dim, 20, fake, need - 1, None) == E
    assert lib.rl_grid_sort(fake, M, dim, 20, None, need, None) == E
    assert lib.rl_grid_sort(None, M, dim, 20, fake, need, None) == E
    # heads
    assert lib.rl_grid_heads(0, dim, fake, fake, fake, need, None) == E
    assert lib.rl_grid_heads(M, dim, None, fake, fake, need, None) == E
    assert lib.rl_grid_heads(M, dim, fake, None, fake, need, None) == E
    assert lib.rl_grid_heads(M, dim, fake, fake, fake, need - 1, None) == E
    assert lib.rl_grid_heads(M, dim, fake, fake, fake + 8, need, None) == E
    # reduce
    assert lib.rl_grid_reduce(fake, M, dim, None, 0, 0, fake, None, fake, fake, need, None) == E
    assert b"V=0" in lib.rl_last_error()
    assert lib.rl_grid_reduce(fake, M, dim, None, 0, M + 1, fake, None, fake, fake, need, None) == E
    assert lib.rl_grid_reduce(fake, M, dim, fake, 0, 10, fake, fake, fake, fake, need, None) == E
    assert b"n_classes" in lib.rl_last_error()
    assert lib.rl_grid_reduce(fake, M, dim, fake, 4, 10, fake, None, fake, fake, need, None) == E
    assert lib.rl_grid_reduce(fake, M, dim, None, 0, 10, None, None, fake, fake, need, None) == E
    assert lib.rl_grid_reduce(fake, M, dim, None, 0, 10, fake, None, fake, fake, need - 1, None) == E
    # confusion
    assert lib.rl_scene_confusion(fake, 10, 0, fake, M, fake, fake, None) == E
    assert b"C=0" in lib.rl_last_error()
    assert lib.rl_scene_confusion(fake, 0, 3, fake, M, fake, fake, None) == E
    assert lib.rl_scene_confusion(fake, 10, 3, fake, 0, fake, fake, None) == E
    assert lib.rl_scene_confusion(fake, 10, 3, fake, M, None, fake, None) == E        # no inverse: V must be M
    assert b"without inverse" in lib.rl_last_error()
    assert lib.rl_scene_confusion(None, 10, 3, fake, M, fake, fake, None) == E
    assert lib.rl_scene_confusion(fake, 10, 3, None, M, fake, fake, None) == E
    assert lib.rl_scene_confusion(fake, 10, 3, fake, M, fake, None, None) == E
