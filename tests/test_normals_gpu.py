"""Normals and curvature on the MI355X: csrc/normals.hip against the numpy twin (utils/normals.py) on every case of
tests/normals_inputs.py, bit for bit; the chunked queries; rl_batch_assemble's rotation of a direction triple
(rl_cloud_job.normal_col) against the float64 product; and the `normals=` keyword of the Model's scene functions."""

import numpy as np
import pytest
import torch

import normals_inputs as ni

pytestmark = pytest.mark.gpu
F32 = np.float32


def _dev():
    return torch.device("cuda", 0)


def _device_normals(xyz, k, vp, **kw):
    from randlanet import _ops as ops
    with torch.cuda.device(_dev()), torch.no_grad():
        out = ops.estimate_normals(torch.from_numpy(np.array(xyz)).to(_dev()), k, vp, **kw)
        return tuple(t.cpu().numpy() for t in out)


# ------------------------------------------------------------------------------------------------ (a) kernel against twin
@pytest.mark.parametrize("name", ni.CASES)
def test_device_equals_the_twin(name):
    from randlanet import _hip
    from randlanet.utils.normals import NormalResult, estimate_normals
    xyz, k, vp = ni.case(name)
    n, c, cov = _device_normals(xyz, k, vp, return_cov=True)
    assert _hip.lib().rl_last_kernel() == b"normals_kernel"
    ni.assert_same(NormalResult(n, c), ni.twin(name), name)
    want = ni.covariances(name.rsplit("-", 1)[0])
    assert cov.dtype == np.float64 and np.array_equal(cov.view(np.uint64), want.view(np.uint64)), name
    ni.assert_same(estimate_normals(xyz, k, vp, device=_dev()), ni.twin(name), name)


def test_default_device_and_features():
    from randlanet.utils.normals import estimate_normals, normal_features
    xyz, k, vp = ni.case("surface_1000-origin")
    want = ni.twin("surface_1000-origin")
    ni.assert_same(estimate_normals(xyz.astype(np.float64), k, vp), want)        # device=None: a GPU is available
    f = normal_features(xyz, k, vp)
    assert f.shape == (1000, 4) and f.dtype == F32 and np.array_equal(f[:, :3], want.normals)
    assert np.array_equal(f[:, 3], want.curvature)


# ------------------------------------------------------------------------------------------------ (b) chunking
@pytest.mark.parametrize("name,chunk", [("surface_1000-origin", 256),      # three full chunks and a ragged one of 232
                                        ("offset_1e3-up", 700),             # above the grid threshold, a single chunk
                                        ("noise_300_k64-origin", 64)])      # the brute-force search, ragged at 44
def test_chunks_do_not_show(name, chunk):
    from randlanet.utils.normals import NormalResult
    xyz, k, vp = ni.case(name)
    whole = _device_normals(xyz, k, vp, return_cov=True)
    parts = _device_normals(xyz, k, vp, chunk=chunk, return_cov=True)
    for a, b in zip(whole, parts):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    ni.assert_same(NormalResult(*parts[:2]), ni.twin(name), name)


def test_entry_refuses_bad_arguments():
    from randlanet import _hip as H
    lib = H.lib()
    with torch.cuda.device(_dev()):
        xyz = torch.zeros((100, 3), device=_dev())
        idx = torch.zeros((100, 8), dtype=torch.int64, device=_dev())
        n, c = torch.zeros((100, 3), device=_dev()), torch.zeros(100, device=_dev())
        torch.cuda.synchronize()
        before = lib.rl_launch_count()
        good = [xyz.data_ptr(), 100, idx.data_ptr(), 0, 100, 8, None, n.data_ptr(), c.data_ptr(), None, None]
        for pos, value in ((0, None), (2, None), (7, None), (8, None), (1, 7), (1, 2 ** 31 - 1), (3, -1), (3, 1), (4, 0),
                           (4, 101), (5, 2), (5, 65)):
            args = list(good)
            args[pos] = value
            assert lib.rl_normals(*args) == H.ERR_ARGS, (pos, value)
        assert lib.rl_launch_count() == before
        assert lib.rl_normals(*good) == 0 and lib.rl_launch_count() == before + 1
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ (c) rl_batch_assemble
B_, N_, F_ = 2, 64, 5


def _assemble(normal_col, augment, pinned=False):
    """One rl_batch_assemble call over two clouds of 200 points with fixed draws; the job records in device memory, as the
    loaders keep them, or in pinned host memory.  Returns (rc, input (B, n, 3 + F), labels, error words, launches)."""
    from randlanet import _hip as H
    from randlanet.utils.augmentation import _rotation
    lib, dev = H.lib(), _dev()
    rs = np.random.RandomState(5)
    src = [(rs.uniform(-2, 2, (200, 3)).astype(F32), rs.standard_normal((200, F_)).astype(F32),
            rs.randint(0, 9, 200).astype(np.int64)) for _ in range(B_)]
    idx = np.stack([rs.permutation(200)[:N_] for _ in range(B_)]).astype(np.int64)
    noise = rs.standard_normal((B_, N_, 3))
    Rs = [_rotation(0.3, -0.2, 0.5), _rotation(-0.1, 0.4, -0.6)]
    with torch.cuda.device(dev):
        keep = [[torch.from_numpy(a).to(dev) for a in cloud] for cloud in src]
        jobs = (H.CloudJob * B_)()
        for b, job in enumerate(jobs):
            job.xyz, job.features, job.labels = (t.data_ptr() for t in keep[b])
            job.n_points, job.xyz_f64, job.normalization, job.augment, job.normal_col = 200, 0, 0, augment, normal_col
            job.jitter_variance, job.jitter_limit, job.scale = 0.01, 0.05, 1.1
            for i in range(9):
                job.R[i] = float(Rs[b].flat[i])
            for i in range(3):
                job.shift[i] = 0.05 * (i - 1)
        raw = torch.from_numpy(np.frombuffer(bytes(jobs), dtype=np.uint8).copy())
        jobs_t = raw.pin_memory() if pinned else raw.to(dev)
        idx_d, noise_d = torch.from_numpy(idx).to(dev), torch.from_numpy(noise).to(dev)
        scratch = torch.zeros(lib.rl_batch_assemble_scratch_doubles(B_, N_), dtype=torch.float64, device=dev)
        inp = torch.full((B_, N_, 3 + F_), -7.0, dtype=torch.float32, device=dev)
        lab = torch.full((B_, N_), -7, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        before = lib.rl_launch_count()
        rc = lib.rl_batch_assemble(jobs_t.data_ptr(), B_, N_, F_, idx_d.data_ptr(), noise_d.data_ptr(), scratch.data_ptr(),
                                   inp.data_ptr(), lab.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        launches = lib.rl_launch_count() - before
        torch.cuda.synchronize()
        words = [int(scratch.view(torch.int32)[lib.rl_batch_assemble_flag_u32(B_, N_, b)].item()) for b in range(B_)]
    picked = np.stack([src[b][1][idx[b]] for b in range(B_)])
    return rc, inp.cpu().numpy(), lab.cpu().numpy(), words, launches, picked, Rs


@pytest.mark.parametrize("pinned", [False, True])
def test_batch_assemble_rotates_the_triple(pinned):
    rc0, inp0, lab0, words0, launches0, picked, Rs = _assemble(0, 1, pinned)
    rc, inp, lab, words, launches, _, _ = _assemble(2, 1, pinned)
    assert rc0 == rc == 0 and words0 == words == [0, 0] and launches0 == launches == 2
    assert np.array_equal(inp0[:, :, 3:], picked)                                  # normal_col = 0: features as they are
    # coordinates, labels and the two other feature columns: the same bits as with normal_col = 0
    assert np.array_equal(inp[:, :, :3].view(np.uint32), inp0[:, :, :3].view(np.uint32)) and np.array_equal(lab, lab0)
    assert np.array_equal(inp[:, :, [3, 7]].view(np.uint32), inp0[:, :, [3, 7]].view(np.uint32))
    assert not np.array_equal(inp[:, :, :3], np.full_like(inp[:, :, :3], -7.0))
    # the triple: the float64 product, rounded once
    for b in range(B_):
        t, R = picked[b][:, 1:4].astype(np.float64), Rs[b]
        want = np.stack([(t[:, 0] * R[r, 0] + t[:, 1] * R[r, 1]) + t[:, 2] * R[r, 2] for r in range(3)], axis=1).astype(F32)
        assert np.array_equal(inp[b][:, 4:7].view(np.uint32), want.view(np.uint32)), b
        assert np.allclose(np.linalg.norm(want, axis=1), np.linalg.norm(t, axis=1), rtol=1e-6)       # a rotation
    # without augmentation the triple is untouched
    rc, inp, lab, words, _, _, _ = _assemble(2, 0, pinned)
    assert rc == 0 and words == [0, 0] and np.array_equal(inp[:, :, 3:], picked)


def test_batch_assemble_refuses_a_triple_that_does_not_fit():
    """normal_col = 4 with F = 5: 3 + 4 - 1 > 5.  Records the host can read are refused before any launch; records in
    device memory - which the entry cannot read without waiting for the stream - are refused by the kernel: the cloud's
    error word, and the features go out as they are.  The loaders refuse on the host either way."""
    from randlanet import _hip as H
    from randlanet.utils.device_dataset import DeviceDataLoader
    rc, inp, _, _, launches, _, _ = _assemble(4, 1, pinned=True)
    assert rc == H.ERR_ARGS and launches == 0
    assert b"normal_col 4 does not fit F=5" in H.lib().rl_last_error()
    assert (inp == -7.0).all()                                                     # nothing ran
    rc, _, _, _, launches, _, _ = _assemble(-1, 1, pinned=True)
    assert rc == H.ERR_ARGS and launches == 0
    rc, inp, _, words, _, picked, _ = _assemble(4, 1, pinned=False)
    assert rc == 0 and words == [2, 2] and np.array_equal(inp[:, :, 3:], picked)
    rs = np.random.RandomState(0)
    ds = [(rs.rand(300, 3).astype(F32), rs.rand(300, F_).astype(F32), np.zeros(300, np.int64))]
    with pytest.raises(ValueError, match="normal_column=3"):
        DeviceDataLoader(ds, 64, 1, device="cuda", normal_column=3)


def test_device_loaders_turn_normals_with_the_cloud():
    from randlanet.utils.augmentation import AugmentationSettings
    from randlanet.utils.device_dataset import DeviceDataLoader
    from randlanet.utils.scene_loader import get_scene_crop_loader
    rs = np.random.RandomState(2)
    M = 3000
    xyz = rs.uniform(0, 3, (M, 3)).astype(F32)
    nrm = rs.standard_normal((M, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    feat = np.concatenate([rs.rand(M, 1).astype(F32), nrm], axis=1)
    ds = [(xyz, feat, np.arange(M, dtype=np.int64))]
    aug = AugmentationSettings(rotation_angle_variances=(0.5, 0.5, 0.5), rotation_angle_limits=(1.0, 1.0, 1.0))
    for make in (lambda c: DeviceDataLoader(ds, 1024, 1, consistent_sampling=False, augmentation_settings=aug,
                                            device="cuda", normal_column=c),
                 lambda c: get_scene_crop_loader(ds, 1024, 1, 1, augmentation_settings=aug, device="cuda", normal_column=c)):
        outs = []
        for c in (None, 1):
            np.random.seed(6)
            torch.manual_seed(6)
            inp, lab, _ = next(iter(make(c)))
            outs.append((inp[0].cpu().numpy(), lab[0].cpu().numpy()))
        (a, la), (b, lb) = outs
        assert np.array_equal(la, lb) and np.array_equal(a[:, :4], b[:, :4])           # the same crop, the same coordinates
        assert np.array_equal(a[:, 4:], nrm[la]) and not np.array_equal(a[:, 4:], b[:, 4:])
        # the triple turned as the cloud did: the rotation that maps the centred source crop onto the centred output
        src, out = xyz[la].astype(np.float64), b[:, :3].astype(np.float64)
        R = np.linalg.lstsq(src - src.mean(0), out - out.mean(0), rcond=None)[0].T
        R /= np.cbrt(np.linalg.det(R))                                               # (the fit carries the scale draw)
        assert np.allclose(b[:, 4:], nrm[la].astype(np.float64) @ R.T, atol=5e-3)
        assert np.allclose(np.linalg.norm(b[:, 4:], axis=1), 1.0, atol=1e-6)


# ------------------------------------------------------------------------------------------------ (d), (e) Model
def _model(use_gpu=True):
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    return Model(RandLANetSettings(n_classes=3, n_points=2048, n_neighbors=8, layer_sizes=[8, 16, 32, 32], n_features=4),
                 use_gpu=use_gpu)


@pytest.fixture(scope="module")
def gpu_model():
    model = _model()
    assert model.device.type == "cuda"
    return model


@pytest.fixture(scope="module")
def scan():
    rs = np.random.RandomState(21)
    return rs.uniform(0, 5, (6000, 3)).astype(F32)


def test_predict_scene_estimates_what_the_caller_would(gpu_model, scan):
    from randlanet.utils.grid import grid_subsample
    from randlanet.utils.normals import normal_features
    kw = dict(votes=1, batch_size=4, seed=2)
    vp = (2.5, 2.5, 9.0)
    np.random.seed(5)
    got = gpu_model.predict_scene(scan, normals=8, viewpoint=vp, **kw)
    np.random.seed(5)
    want = gpu_model.predict_scene(scan, normal_features(scan, 8, vp), **kw)
    assert got.shape == (3, 6000) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # with grid: estimated on the representatives, carried to the raw points through `inverse`
    sub = grid_subsample(scan, cell=0.25, device=_dev())
    assert 2048 < sub.xyz.shape[0] < 6000
    np.random.seed(5)
    got = gpu_model.predict_scene(scan, normals=8, grid=0.25, **kw)
    np.random.seed(5)
    want = gpu_model.predict_scene(sub.xyz, normal_features(sub.xyz, 8), **kw)[:, sub.inverse]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the caller's own features come first
    own = np.random.RandomState(1).rand(6000, 1).astype(F32)
    with pytest.raises(AssertionError, match="Input should have shape"):
        gpu_model.predict_scene(scan, own, normals=8, **kw)
    with pytest.raises(ValueError, match="must be an integer in 3 .. 64"):
        gpu_model.predict_scene(scan, normals=2, **kw)
    with pytest.raises(ValueError, match="viewpoint"):
        gpu_model.predict_scene(scan, normals=8, viewpoint=(0, 0), **kw)


def test_predict_scenes_evaluate_and_instances_take_normals(gpu_model, scan):
    from randlanet.utils.normals import normal_features
    kw = dict(votes=1, batch_size=4, seed=2)
    scenes = [(scan, None), (scan[:3000] + F32(1.0), None)]
    np.random.seed(5)
    got = gpu_model.predict_scenes(scenes, normals=8, **kw)
    np.random.seed(5)
    want = gpu_model.predict_scenes([(x, normal_features(x, 8)) for x, _ in scenes], **kw)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and [g.shape for g in got] == [(3, 6000), (3, 3000)]
    with pytest.raises(ValueError, match="scene 1 has 5 points, fewer than the normals=k=8"):
        gpu_model.predict_scenes([scenes[0], (scan[:5], None)], normals=8, pad_small_scenes=True, **kw)
    labels = (scan[:, 2] > 2.5).astype(np.int64)
    np.random.seed(5)
    m1, c1 = gpu_model.evaluate_scenes([(scan, None, labels)], normals=8, return_confusion=True, **kw)
    np.random.seed(5)
    m2, c2 = gpu_model.evaluate_scenes([(scan, normal_features(scan, 8), labels)], return_confusion=True, **kw)
    assert np.array_equal(c1, c2) and c1.sum() == 6000
    np.random.seed(5)
    res = gpu_model.predict_instances(scan, radius=0.3, min_points=3, ignore_classes=(), normals=8, **kw)
    np.random.seed(5)
    ref = gpu_model.predict_instances(scan, normal_features(scan, 8), radius=0.3, min_points=3, ignore_classes=(), **kw)
    assert res.instance.shape == (6000,) and res.count.shape[0] >= 1
    assert all(np.array_equal(a, b) for a, b in zip(res, ref))


def test_cpu_placed_model_gives_the_same_normals(gpu_model, scan):
    cpu_model = _model(use_gpu=False)
    assert cpu_model.device.type == "cpu"
    for vp in (None, (0.0, 0.0, 0.0)):
        a = gpu_model._scene_path.append_normals(scan, 8, vp, "the scene")
        b = cpu_model._scene_path.append_normals(scan, 8, vp, "the scene")
        assert torch.is_tensor(a) and a.is_cuda and isinstance(b, np.ndarray) and b.shape == (6000, 7)
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.view(np.uint32))
    with pytest.raises(ValueError, match="the scene has 7 points, fewer than the normals=k=8"):
        cpu_model.predict_scene(scan[:7], normals=8, pad_small_scenes=True)


def _train(train, val, **kw):
    from randlanet import AugmentationSettings, TrainingSettings
    torch.manual_seed(0)
    np.random.seed(0)
    model = _model()
    model.train_scenes(train, val, TrainingSettings(epochs=1, batch_size=2, learning_rate=1e-2, early_stopping=False),
                       AugmentationSettings(), crops_per_epoch=4, validation_crops=2, center_noise=0.05, seed=3,
                       class_names=["a", "b", "c"], normals=8, **kw)
    return model


def test_train_scenes_with_normals_is_reproducible():
    rs = np.random.RandomState(8)

    def scene(M):
        xyz = rs.uniform((0, 0, -1), (4, 4, 1), (M, 3)).astype(F32)
        return xyz, np.zeros((M, 0), F32), (xyz[:, 2] > 0).astype(np.int64)

    train, val = [scene(5000), scene(3000)], [scene(3000)]
    m1, m2 = _train(train, val, viewpoint=(2.0, 2.0, 6.0)), _train(train, val, viewpoint=(2.0, 2.0, 6.0))
    moved = False
    fresh = _model().module.state_dict()
    for (k, a), b in zip(m1.module.state_dict().items(), m2.module.state_dict().values()):
        assert torch.equal(a, b), k
        moved = moved or not torch.equal(a.cpu(), fresh[k].cpu())
    assert moved
    with pytest.raises(ValueError, match="training scene 1 has 7 points, fewer than the normals=k=8"):
        _train([train[0], tuple(a[:7] for a in train[1])], val, pad_small_scenes=True)
    with pytest.raises(ValueError, match="validation scene 0 has 7 points, fewer than the normals=k=8"):
        _train(train, [tuple(a[:7] for a in val[0])], pad_small_scenes=True)
