"""Statistical outlier removal on the host: the numpy twin (utils/outliers.py) against the all-pairs yardstick of
tests/outliers_inputs.py, bit for bit; what the filter does to a surface with spikes; the refusals; and the `outliers=`
keyword of a CPU-placed Model's scene functions against the same steps done by hand."""
import numpy as np
import pytest
import torch

import outliers_inputs as oi

F32 = np.float32


# ------------------------------------------------------------------------------------------------ 1. twin against yardstick
@pytest.mark.parametrize("name", oi.ALL_PAIRS)
def test_twin_equals_all_pairs(name):
    got, want = oi.twin(name), oi.yardstick(name)
    oi.assert_same(got, want, name)
    M = oi.case(name)[0].shape[0]
    assert got.keep.shape == (M,) and got.kept.shape == (int(got.keep.sum()),)
    assert np.array_equal(got.slot[got.kept], np.arange(got.kept.shape[0])) and (got.slot[~got.keep] == -1).all()


def test_the_sum_order_is_part_of_the_result():
    """A plain left-to-right sum is not the fixed sum: the statistics have to be compared as bits, not through the mask."""
    differs = 0
    for seed in (1, 2, 3):
        res = oi.twin(f"surface_spikes_{seed}")
        plain = 0.0
        for v in res.mean_distance.tolist():
            plain += v
        differs += oi.bits(np.float64(plain) / np.float64(1012))[0] != oi.bits(res.mean)[0]
    assert differs >= 1


# ------------------------------------------------------------------------------------------------ 2. behaviour
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_spikes_are_removed_and_nothing_else(seed):
    xyz, is_spike = oi.spikes(seed)
    res = oi.twin(f"surface_spikes_{seed}")
    assert np.array_equal(xyz, oi.case(f"surface_spikes_{seed}")[0])
    assert is_spike.sum() == oi.N_SPIKES and np.array_equal(~res.keep, is_spike)
    print("smallest |m - t|:", np.abs(res.mean_distance - res.threshold).min())      # (about 0.1: no point sits on it)


def test_coincident_points_are_all_kept():
    res = oi.twin("coincident")
    assert res.mean == 0.0 and res.std == 0.0 and res.threshold == 0.0 and (res.mean_distance == 0.0).all()
    assert res.keep.all() and np.array_equal(res.kept, np.arange(50)) and np.array_equal(res.slot, np.arange(50))


def test_smallest_cloud():
    xyz, k, _ = oi.case("smallest")
    res = oi.twin("smallest")
    d = np.sqrt(((xyz[:, None].astype(np.float64) - xyz[None].astype(np.float64)) ** 2).sum(-1))
    assert np.allclose(res.mean_distance, d.sum(1) / k, rtol=1e-6)


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals():
    from randlanet.utils.outliers import remove_statistical_outliers, statistical_outliers, statistical_outliers_host
    xyz = np.array(oi.case("below_grid_k3")[0])
    for fn in (statistical_outliers_host, lambda *a, **kw: statistical_outliers(*a, device="cpu", **kw)):
        for k in (0, 64, -1, 2.5, True, "3", None):
            with pytest.raises(ValueError, match="must be an integer in 1 .. 63"):
                fn(xyz, k=k)
        for r in (-0.5, float("nan"), float("inf"), "x", None):
            with pytest.raises(ValueError, match="std_ratio"):
                fn(xyz, std_ratio=r)
        with pytest.raises(ValueError, match=r"expected \(M, 3\)"):
            fn(xyz[:, :2])
        with pytest.raises(ValueError, match=r"expected \(M, 3\)"):
            fn(xyz.reshape(-1))
        with pytest.raises(ValueError, match="M=16 points, outside k \\+ 1 = 17"):
            fn(xyz[:16], k=16)
        bad = xyz.copy()
        bad[7, 1] = np.nan
        with pytest.raises(ValueError, match="non-finite coordinates, first at point 7"):
            fn(bad)
        big = xyz.astype(np.float64)
        big[9, 2] = 1e39                      # finite in float64, beyond float32
        with pytest.raises(ValueError, match="non-finite coordinates, first at point 9"):
            fn(big)
        far = xyz.copy()
        far[0] = 3e38                         # finite, but every squared distance to it overflows
        with pytest.raises(ValueError, match="squared distance overflows"):
            fn(far, k=3)
    assert statistical_outliers_host(xyz[:17], k=16).keep.shape == (17,)          # M = k + 1 is served
    assert statistical_outliers_host(xyz, k=3.0, std_ratio=0).keep.sum() >= 1      # an integral float, a zero ratio
    with pytest.raises(ValueError, match="column 0 has shape"):
        remove_statistical_outliers(xyz, np.zeros(299), device="cpu")


def test_remove_carries_columns():
    from randlanet.utils.outliers import remove_statistical_outliers
    xyz, k, ratio = oi.case("surface_spikes_2")
    want = oi.twin("surface_spikes_2")
    feat = np.random.RandomState(0).rand(1012, 2).astype(F32)
    labels = np.arange(1012, dtype=np.int64)
    x, f, l, res = remove_statistical_outliers(xyz.astype(np.float64), feat, labels, k=k, std_ratio=ratio, device="cpu")
    oi.assert_same(res, want)
    assert x.dtype == np.float64 and x.shape == (1000, 3) and np.array_equal(x, xyz[want.kept].astype(np.float64))
    assert f.dtype == F32 and np.array_equal(f, feat[want.kept]) and np.array_equal(l, want.kept)
    x, res = remove_statistical_outliers(xyz, k=k, std_ratio=ratio, device="cpu")
    assert np.array_equal(x, xyz[want.kept])


# ------------------------------------------------------------------------------------------------ 4. CPU-placed model
@pytest.fixture(scope="module")
def cpu_model():
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    return Model(RandLANetSettings(n_classes=4, n_points=512, n_neighbors=8, layer_sizes=[8, 16, 32, 32]), use_gpu=False)


KW = dict(votes=1, batch_size=2, seed=2)


def test_model_refusals_come_before_any_work(cpu_model):
    xyz = oi.case("surface_spikes_1")[0]
    for bad, match in (((0, 2.0), "must be an integer in 1 .. 63"), ((16, -1.0), "std_ratio"), ((16,), "must be a pair"),
                       (16, "must be a pair")):
        for fn in (cpu_model.predict_scene, lambda *a, **kw: cpu_model.predict_instances(*a, radius=0.1, **kw),
                   lambda *a, **kw: cpu_model.predict_keypoints(*a, radius=0.1, **kw)):
            with pytest.raises(ValueError, match=match):
                fn(xyz, outliers=bad, **KW)
    with pytest.raises(ValueError, match="the scene has 16 points, fewer than the k \\+ 1 = 17"):
        cpu_model.predict_scene(xyz[:16], outliers=(16, 2.0), pad_small_scenes=True, **KW)


def test_predict_scene_equals_the_steps_by_hand(cpu_model):
    xyz = oi.case("surface_spikes_1")[0]
    res = oi.twin("surface_spikes_1")
    np.random.seed(5)
    got, count, removed = cpu_model.predict_scene(xyz, outliers=(16, 2.0), return_counts=True, return_outliers=True, **KW)
    np.random.seed(5)
    p, c = cpu_model.predict_scene(xyz[res.kept], return_counts=True, **KW)
    want, wcount = np.zeros((4, 1012), F32), np.zeros(1012, c.dtype)
    want[:, res.kept], wcount[res.kept] = p, c
    assert np.array_equal(removed, ~res.keep) and removed.dtype == np.bool_ and removed.sum() == oi.N_SPIKES
    assert got.dtype == F32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert count.dtype == c.dtype and np.array_equal(count, wcount) and (count[~removed] >= 1).all()
    # without the keyword nothing changes, and the mask of return_outliers is empty
    np.random.seed(5)
    a = cpu_model.predict_scene(xyz, **KW)
    np.random.seed(5)
    b, none = cpu_model.predict_scene(xyz, return_outliers=True, **KW)
    assert np.array_equal(a, b) and none.shape == (1012,) and not none.any()
    np.random.seed(5)
    only = cpu_model.predict_scene(xyz, outliers=(16, 2.0), **KW)
    assert isinstance(only, np.ndarray) and np.array_equal(only.view(np.uint32), want.view(np.uint32))


def test_predict_scene_with_grid_filters_the_representatives(cpu_model):
    from randlanet.utils.grid import grid_subsample_host
    from randlanet.utils.outliers import statistical_outliers_host
    rs = np.random.RandomState(4)
    xyz = np.concatenate([oi.case("surface_spikes_3")[0], oi.case("surface_spikes_3")[0] + F32(0.004) * rs.randn(1012, 3)
                          .astype(F32)])
    sub = grid_subsample_host(xyz, None, cell=0.05)
    res = statistical_outliers_host(sub.xyz, 8, 1.5)
    V, Vk = sub.xyz.shape[0], res.kept.shape[0]
    assert 512 < Vk < V < 2024
    np.random.seed(5)
    got, removed = cpu_model.predict_scene(xyz, grid=0.05, outliers=(8, 1.5), return_outliers=True, **KW)
    np.random.seed(5)
    p = cpu_model.predict_scene(sub.xyz[res.kept], **KW)
    full = np.zeros((4, V), F32)
    full[:, res.kept] = p
    assert np.array_equal(removed, ~res.keep[sub.inverse]) and 0 < removed.sum() < 2024
    assert np.array_equal(got.view(np.uint32), full[:, sub.inverse].view(np.uint32))
    assert (got[:, removed] == 0).all() and np.allclose(got[:, ~removed].sum(0), 1.0, atol=1e-5)


def test_predict_instances_and_keypoints_leave_the_removed_points_out(cpu_model):
    xyz = oi.case("surface_spikes_1")[0]
    res = oi.twin("surface_spikes_1")
    kw = dict(radius=0.15, min_points=3, ignore_classes=(), **KW)
    np.random.seed(5)
    got = cpu_model.predict_instances(xyz, outliers=(16, 2.0), **kw)
    np.random.seed(5)
    ref = cpu_model.predict_instances(xyz[res.kept], **kw)
    assert got.instance.shape == (1012,) and got.label.shape == (1012,) and ref.count.shape[0] >= 1
    assert (got.instance[~res.keep] == -1).all() and (got.label[~res.keep] == -1).all()
    assert np.array_equal(np.flatnonzero(got.label == -1), np.flatnonzero(~res.keep))
    assert np.array_equal(got.instance[res.kept], ref.instance) and np.array_equal(got.label[res.kept], ref.label)
    assert all(np.array_equal(a, b) for a, b in zip(got[2:], ref[2:]))
    kw = dict(radius=0.3, min_score=0.0, ignore_classes=(), **KW)
    np.random.seed(5)
    kp = cpu_model.predict_keypoints(xyz, outliers=(16, 2.0), **kw)
    np.random.seed(5)
    kref = cpu_model.predict_keypoints(xyz[res.kept], **kw)
    assert kp.index.shape[0] >= 1 and res.keep[kp.index].all()
    assert np.array_equal(kp.index, res.kept[kref.index])
    assert all(np.array_equal(a, b) for a, b in zip(kp[1:], kref[1:]))
