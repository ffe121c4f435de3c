"""Statistical outlier removal on the MI355X: csrc/outliers.hip against the numpy twin (utils/outliers.py) on every case of
tests/outliers_inputs.py, bit for bit; the chunked queries; the entries' refusals and workspace; and the `outliers=` keyword
of a GPU-placed Model's scene functions against the same steps done by hand on the device path."""
import numpy as np
import pytest
import torch

import outliers_inputs as oi

pytestmark = pytest.mark.gpu
F32 = np.float32


def _dev():
    return torch.device("cuda", 0)


def _device_outliers(xyz, k, ratio, **kw):
    from randlanet import _ops as ops
    from randlanet.utils.outliers import OutlierResult
    with torch.cuda.device(_dev()), torch.no_grad():
        keep, slot, kept, m, stats = ops.statistical_outliers(torch.from_numpy(np.array(xyz)).to(_dev()), k, ratio, **kw)
        return OutlierResult(keep.cpu().numpy(), kept.cpu().numpy(), slot.cpu().numpy(), m.cpu().numpy(),
                             *(np.float64(s) for s in stats))


# ------------------------------------------------------------------------------------------------ (a) kernels against twin
@pytest.mark.parametrize("name", oi.CASES)
def test_device_equals_the_twin(name):
    from randlanet import _hip
    from randlanet.utils.outliers import statistical_outliers
    xyz, k, ratio = oi.case(name)
    got = _device_outliers(xyz, k, ratio)
    assert _hip.lib().rl_last_kernel() == b"ol_write"
    oi.assert_same(got, oi.twin(name), name)
    oi.assert_same(statistical_outliers(xyz, k, ratio, device=_dev()), oi.twin(name), name)


def test_default_device_and_remove():
    from randlanet.utils.outliers import remove_statistical_outliers, statistical_outliers
    xyz, k, ratio = oi.case("surface_spikes_2")
    want = oi.twin("surface_spikes_2")
    oi.assert_same(statistical_outliers(xyz.astype(np.float64), k, ratio), want)      # device=None: a GPU is available
    x, lab, res = remove_statistical_outliers(xyz, np.arange(1012), k=k, std_ratio=ratio)
    oi.assert_same(res, want)
    assert np.array_equal(x, xyz[want.kept]) and np.array_equal(lab, want.kept)
    far = np.array(xyz)
    far[0] = 3e38                                     # every squared distance to it overflows: found on the device
    with pytest.raises(ValueError, match="squared distance overflows"):
        statistical_outliers(far, k, ratio, device=_dev())


# ------------------------------------------------------------------------------------------------ (b) chunking
@pytest.mark.parametrize("name,chunk", [("surface_spikes_1", 256),         # three full chunks and a ragged one of 244
                                        ("below_grid_k63", 64),             # the brute-force search, ragged at 44
                                        ("below_grid_k3", 64)])
def test_chunks_do_not_show(name, chunk):
    xyz, k, ratio = oi.case(name)
    whole = _device_outliers(xyz, k, ratio)
    parts = _device_outliers(xyz, k, ratio, chunk=chunk)
    for a, b in zip(whole, parts):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)), name
    oi.assert_same(parts, oi.twin(name), name)


# ------------------------------------------------------------------------------------------------ (c) the entries
def test_entries_refuse_bad_arguments():
    from randlanet import _hip as H
    lib = H.lib()
    with torch.cuda.device(_dev()):
        M, k = 100, 8
        d2 = torch.rand((M, k + 1), device=_dev()).sort(dim=1).values.contiguous()
        mean = torch.zeros(M, dtype=torch.float64, device=_dev())
        keep = torch.zeros(M, dtype=torch.uint8, device=_dev())
        slot = torch.zeros(M, dtype=torch.int32, device=_dev())
        kept = torch.zeros(M, dtype=torch.int64, device=_dev())
        stats = torch.zeros(4, dtype=torch.float64, device=_dev())
        need = lib.rl_outliers_workspace_bytes(M)
        ws = torch.zeros(need + 256, dtype=torch.uint8, device=_dev())
        torch.cuda.synchronize()
        before = lib.rl_launch_count()
        good = [d2.data_ptr(), M, 0, M, k, mean.data_ptr(), None]
        for pos, value in ((0, None), (5, None), (1, k), (1, 2 ** 31 - 1), (2, -1), (2, 1), (3, 0), (3, M + 1), (4, 0),
                           (4, 64), (4, -3)):
            args = list(good)
            args[pos] = value
            assert lib.rl_outliers_mean_distance(*args) == H.ERR_ARGS, (pos, value)
        good_f = [mean.data_ptr(), M, 2.0, keep.data_ptr(), slot.data_ptr(), kept.data_ptr(), stats.data_ptr(),
                  ws.data_ptr(), need, None]
        for pos, value in ((0, None), (3, None), (4, None), (5, None), (6, None), (7, None), (1, 1), (1, 2 ** 31 - 1),
                           (2, -1.0), (2, float("nan")), (2, float("inf")), (7, ws.data_ptr() + 8), (8, need - 1), (8, 0)):
            args = list(good_f)
            args[pos] = value
            assert lib.rl_outliers_filter(*args) == H.ERR_ARGS, (pos, value)
        # the two halves of the filter on their own: the same refusals
        good_t, good_c = good_f[:3] + good_f[6:], good_f[:2] + good_f[3:]
        for pos, value in ((0, None), (3, None), (4, None), (1, 1), (2, -1.0), (2, float("nan")), (5, need - 1)):
            args = list(good_t)
            args[pos] = value
            assert lib.rl_outliers_threshold(*args) == H.ERR_ARGS, (pos, value)
        for pos, value in ((0, None), (2, None), (3, None), (4, None), (5, None), (6, None), (1, 2 ** 31 - 1), (7, need - 1)):
            args = list(good_c)
            args[pos] = value
            assert lib.rl_outliers_compact(*args) == H.ERR_ARGS, (pos, value)
        assert lib.rl_launch_count() == before
        assert lib.rl_outliers_mean_distance(*good) == 0 and lib.rl_launch_count() == before + 1
        assert lib.rl_last_kernel() == b"ol_mean"
        assert lib.rl_outliers_filter(*good_f) == 0 and lib.rl_launch_count() == before + 8
        assert lib.rl_last_kernel() == b"ol_write"
        torch.cuda.synchronize()
        # what the two entries wrote, against the twin's two halves on the same distances
        from randlanet.utils.outliers import filter_host, mean_distances
        want = filter_host(mean_distances(d2.cpu().numpy(), k), 2.0)
        assert np.array_equal(oi.bits(mean.cpu().numpy()), oi.bits(want.mean_distance))
        assert np.array_equal(oi.bits(stats.cpu().numpy()[:3]), oi.bits([want.mean, want.std, want.threshold]))
        n = int(stats[3].item())
        assert n == want.kept.shape[0] and np.array_equal(kept[:n].cpu().numpy(), want.kept)
        assert np.array_equal(keep.cpu().numpy().astype(bool), want.keep) and np.array_equal(slot.cpu().numpy(), want.slot)


def test_workspace_bytes():
    from randlanet import _hip
    lib = _hip.lib()
    for M in (-1, 0, 1, 2 ** 31 - 1, 2 ** 40):
        assert lib.rl_outliers_workspace_bytes(M) == 0, M
    last = 0
    for M in (2, 63, 64, 1023, 1024, 1025, 70000, 10 ** 7, 2 ** 31 - 2):
        n = lib.rl_outliers_workspace_bytes(M)
        chunks = -(-M // 1024)
        assert n >= 32 + 12 * chunks and n % 256 == 0 and n >= last, M      # the statistics, a double and a count per chunk
        assert n <= 768 + 12 * chunks, M
        last = n


# ------------------------------------------------------------------------------------------------ (d) Model
def _model(use_gpu=True, n_features=0):
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    return Model(RandLANetSettings(n_classes=3, n_points=2048, n_neighbors=8, layer_sizes=[8, 16, 32, 32],
                                   n_features=n_features), use_gpu=use_gpu)


@pytest.fixture(scope="module")
def gpu_model():
    model = _model()
    assert model.device.type == "cuda"
    return model


@pytest.fixture(scope="module")
def scan():
    """6000 points in a slab and 40 floating above it."""
    rs = np.random.RandomState(21)
    xyz = np.concatenate([rs.uniform((0, 0, 0), (5, 5, 2.5), (6000, 3)), rs.uniform((0, 0, 4), (5, 5, 8), (40, 3))])
    return np.ascontiguousarray(xyz[rs.permutation(6040)], dtype=F32)


@pytest.fixture(scope="module")
def filtered(scan):
    from randlanet.utils.outliers import statistical_outliers_host
    res = statistical_outliers_host(scan, 8, 2.0)
    assert 30 <= (~res.keep).sum() < 300
    return res


KW = dict(votes=1, batch_size=4, seed=2)


def test_predict_scene_removes_what_the_caller_would(gpu_model, scan, filtered):
    np.random.seed(5)
    got, count, removed = gpu_model.predict_scene(scan, outliers=(8, 2.0), return_counts=True, return_outliers=True, **KW)
    np.random.seed(5)
    p, c = gpu_model.predict_scene(scan[filtered.kept], return_counts=True, **KW)
    want, wcount = np.zeros((3, 6040), F32), np.zeros(6040, c.dtype)
    want[:, filtered.kept], wcount[filtered.kept] = p, c
    assert np.array_equal(removed, ~filtered.keep)                       # the device's mask is the twin's
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(count, wcount)
    with pytest.raises(ValueError, match="must be an integer in 1 .. 63"):
        gpu_model.predict_scene(scan, outliers=(64, 2.0), **KW)
    with pytest.raises(ValueError, match="the scene has 8 points, fewer than the k \\+ 1 = 9"):
        gpu_model.predict_scene(scan[:8], outliers=(8, 2.0), pad_small_scenes=True, **KW)


def test_predict_scene_with_grid_and_normals(scan):
    from randlanet.utils.grid import grid_subsample
    from randlanet.utils.normals import normal_features
    from randlanet.utils.outliers import statistical_outliers
    model = _model(n_features=4)
    sub = grid_subsample(scan, cell=0.25, device=_dev())
    res = statistical_outliers(sub.xyz, 8, 2.0, device=_dev())
    V, Vk = sub.xyz.shape[0], res.kept.shape[0]
    assert 2048 < Vk < V < 6040
    kept_xyz = np.ascontiguousarray(sub.xyz[res.kept])
    np.random.seed(5)
    got, removed = model.predict_scene(scan, grid=0.25, outliers=(8, 2.0), normals=8, return_outliers=True, **KW)
    np.random.seed(5)
    p = model.predict_scene(kept_xyz, normal_features(kept_xyz, 8), **KW)      # normals of the kept points only
    full = np.zeros((3, V), F32)
    full[:, res.kept] = p
    assert np.array_equal(removed, ~res.keep[sub.inverse]) and removed.any()
    assert np.array_equal(got.view(np.uint32), full[:, sub.inverse].view(np.uint32))
    # without grid: the normals still see the kept points only
    raw = statistical_outliers(scan, 8, 2.0, device=_dev())
    np.random.seed(5)
    got = model.predict_scene(scan, outliers=(8, 2.0), normals=8, **KW)
    np.random.seed(5)
    p = model.predict_scene(scan[raw.kept], normal_features(scan[raw.kept], 8), **KW)
    assert np.array_equal(got[:, raw.kept].view(np.uint32), p.view(np.uint32)) and (got[:, ~raw.keep] == 0).all()


def test_instances_and_keypoints_never_return_a_removed_point(gpu_model, scan, filtered):
    gone = ~filtered.keep
    kw = dict(radius=0.3, min_points=3, ignore_classes=(), **KW)
    np.random.seed(5)
    res = gpu_model.predict_instances(scan, outliers=(8, 2.0), oriented_boxes=True, **kw)
    np.random.seed(5)
    ref = gpu_model.predict_instances(scan[filtered.kept], oriented_boxes=True, **kw)
    assert res.instance.shape == (6040,) and res.count.shape[0] >= 1
    assert (res.instance[gone] == -1).all() and (res.label[gone] == -1).all() and (res.label[~gone] >= 0).all()
    assert np.array_equal(res.instance[filtered.kept], ref.instance) and np.array_equal(res.label[filtered.kept], ref.label)
    assert all(np.array_equal(a, b) for a, b in zip(res[2:], ref[2:]))
    from randlanet.utils.grid import grid_subsample
    from randlanet.utils.outliers import statistical_outliers
    sub = grid_subsample(scan, cell=0.25, device=_dev())
    cells = statistical_outliers(sub.xyz, 8, 2.0, device=_dev())
    away = ~cells.keep[sub.inverse]                         # with grid: every raw point of a removed cell
    np.random.seed(5)
    res = gpu_model.predict_instances(scan, outliers=(8, 2.0), grid=0.25, **kw)
    assert away.sum() >= 30 and (res.instance[away] == -1).all() and (res.label[away] == -1).all()
    assert (res.label[~away] >= 0).all() and (res.instance >= 0).any()
    kw = dict(radius=0.5, min_score=0.0, ignore_classes=(), **KW)
    np.random.seed(5)
    kp = gpu_model.predict_keypoints(scan, outliers=(8, 2.0), **kw)
    np.random.seed(5)
    kref = gpu_model.predict_keypoints(scan[filtered.kept], **kw)
    assert kp.index.shape[0] >= 1 and filtered.keep[kp.index].all()
    assert np.array_equal(kp.index, filtered.kept[kref.index])
    assert all(np.array_equal(a, b) for a, b in zip(kp[1:], kref[1:]))
    np.random.seed(5)
    kp = gpu_model.predict_keypoints(scan, outliers=(8, 2.0), grid=0.25, **kw)
    assert kp.index.shape[0] >= 1 and not away[kp.index].any()


def test_cpu_placed_model_removes_the_same_points(gpu_model, scan, filtered):
    cpu_model = _model(use_gpu=False)
    a, ia = gpu_model._scene_path.remove_outliers(scan, None, (8, 2.0), False, "the scene")
    b, ib = cpu_model._scene_path.remove_outliers(scan, None, (8, 2.0), False, "the scene")
    assert torch.is_tensor(a) and a.is_cuda and isinstance(b, np.ndarray) and b.shape == (filtered.kept.shape[0], 3)
    assert np.array_equal(a.cpu().numpy().view(np.uint32), b.view(np.uint32))
    assert np.array_equal(ia, ib) and np.array_equal(ib, filtered.slot)
