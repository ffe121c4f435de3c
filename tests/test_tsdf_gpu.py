"""TSDF fusion on the MI355X: csrc/tsdf.hip against the numpy twin (utils/tsdf.py) on every case of tests/tsdf_inputs.py, bit
for bit - the state after each frame, M, the points and their edges -; planted states; arrays and frames that are not 16-byte
aligned; the entries' refusals and workspace; and DepthFusion on a GPU model against the same calls on a CPU-placed copy."""
import ctypes

import numpy as np
import pytest
import torch

import tsdf_inputs as ti

pytestmark = pytest.mark.gpu
F32 = np.float32


def _dev():
    return torch.device("cuda", 0)


def _T():
    from randlanet.utils import tsdf
    return tsdf


def _np(t):
    return t.cpu().numpy()


def _last_kernel():
    from randlanet import _hip
    return _hip.lib().rl_last_kernel()


# ------------------------------------------------------------------------------------------------ (a) kernels against twin
@pytest.mark.parametrize("name", ti.CASES)
def test_device_equals_the_twin(name):
    T = _T()
    c = ti.case(name)
    states, cloud = ti.twin(name)
    vol = ti.volume(c, _dev())
    assert torch.is_tensor(vol.tsdf) and vol.tsdf.is_cuda and vol.weight.is_cuda and vol.tsdf.shape == states[0][0].shape
    for k, (depth, pose) in enumerate(c.frames):
        vol.integrate(np.array(depth), c.camera, pose, c.z_range)
        assert _last_kernel() == b"ts_integrate"
        ti.assert_same_state((vol.tsdf, vol.weight), states[k], (name, k))
    got = vol.extract(c.min_weight)
    assert _last_kernel() == (b"ts_write" if cloud.edge.shape[0] else b"ts_scan")
    assert torch.is_tensor(got.xyz) and got.xyz.is_cuda and got.edge.is_cuda and got.xyz.is_contiguous()
    assert got.xyz.shape[0] == cloud.edge.shape[0]                                # M
    ti.assert_same_cloud(got, cloud, name)
    ti.assert_same_state((vol.tsdf, vol.weight), states[-1], name)                # the extraction writes nothing
    if c.max_weight >= 2:
        ti.assert_same_cloud(vol.extract(2), T.extract_host(*states[-1], vol.origin, vol.voxel, 2), (name, 2))
    if name == "outside":
        assert got.xyz.shape == (0, 3) and got.edge.shape == (0,)
    if name == "128x128x80":
        assert cloud.edge.shape[0] > 20000
    vol.reset()
    assert bool((vol.tsdf == 1).all()) and bool((vol.weight == 0).all()) and vol.tsdf.is_cuda


@pytest.mark.parametrize("name", ti.PLANTED)
def test_extraction_of_planted_states(name):
    T = _T()
    t, w, origin, voxel, min_weight, max_weight = ti.planted(name)
    nz, ny, nx = t.shape
    vol = T.TsdfVolume(origin, voxel, (nx, ny, nz), None, max_weight, device=_dev())
    vol.tsdf.copy_(torch.from_numpy(np.array(t)))
    vol.weight.copy_(torch.from_numpy(np.array(w)))
    want = ti.planted_twin(name)
    ti.assert_same_cloud(vol.extract(min_weight), want, name)
    ti.assert_same_cloud(vol.extract(1), T.extract_host(t, w, vol.origin, vol.voxel, 1), (name, 1))
    if name == "random-128x128x80":                  # 1280 chunks, five per thread of the scan, and every one holds points
        assert want.edge.shape[0] > 50000 and np.unique(want.edge // (3 * 1024)).shape[0] == 1280


def test_a_state_that_is_only_4_byte_aligned():
    """tsdf and weight one float into their buffers: every run goes element by element, and nothing around them is written."""
    c = ti.case("13x11x9")
    states, cloud = ti.twin("13x11x9")
    vol = ti.volume(c, _dev())
    V = vol.tsdf.numel()
    pads = [torch.full((V + 9,), fill, dtype=torch.float32, device=_dev()) for fill in (7.0, -7.0)]
    vol.tsdf, vol.weight = (p[1:1 + V].view(vol.shape) for p in pads)
    vol.tsdf.fill_(1.0)
    vol.weight.fill_(0.0)
    assert vol.tsdf.data_ptr() % 16 == 4 and vol.tsdf.is_contiguous()
    for k, (depth, pose) in enumerate(c.frames):
        vol.integrate(np.array(depth), c.camera, pose, c.z_range)
        ti.assert_same_state((vol.tsdf, vol.weight), states[k], k)
    ti.assert_same_cloud(vol.extract(c.min_weight), cloud)
    for p, fill in zip(pads, (7.0, -7.0)):
        around = _np(p)
        assert around[0] == fill and (around[1 + V:] == fill).all()


def test_frames_that_are_only_2_byte_aligned_and_device_frames():
    """Frame 1 of a (2, H, W) tensor with odd H * W gives the bits of the frame uploaded alone, and a device-tensor frame the
    bits of a numpy frame."""
    c = ti.case("odd-frame")
    states, _ = ti.twin("odd-frame")
    both = np.stack([np.array(f) for f, _ in c.frames])
    batch = torch.from_numpy(both).to(_dev())
    assert batch[1].is_contiguous() and batch[1].data_ptr() % 16 == 2
    in_place, alone, host_frames = ti.volume(c, _dev()), ti.volume(c, _dev()), ti.volume(c, _dev())
    for k in (0, 1):
        in_place.integrate(batch[k], c.camera, None, c.z_range)
        alone.integrate(torch.from_numpy(both[k]).to(_dev()), c.camera, None, c.z_range)
        host_frames.integrate(both[k], c.camera, None, c.z_range)
        for vol in (in_place, alone, host_frames):
            ti.assert_same_state((vol.tsdf, vol.weight), states[k], k)
    assert np.array_equal(_np(batch), both)
    # a host volume takes a device frame too
    host = ti.volume(c, "cpu")
    host.integrate(batch[0], c.camera, None, c.z_range)
    ti.assert_same_state((host.tsdf, host.weight), states[0])


def test_a_volume_moves_between_the_placements():
    c = ti.case("13x11x9")
    states, cloud = ti.twin("13x11x9")
    vol = ti.volume(c, "cpu")
    vol.integrate(c.frames[0][0], c.camera, c.frames[0][1], c.z_range)
    assert vol.to(_dev()) is vol and vol.tsdf.is_cuda and vol.device == _dev()
    vol.integrate(np.array(c.frames[1][0]), c.camera, c.frames[1][1], c.z_range)
    ti.assert_same_state((vol.tsdf, vol.weight), states[1])
    vol.to("cpu")
    assert isinstance(vol.tsdf, np.ndarray)
    ti.assert_same_cloud(vol.extract(c.min_weight), cloud)


# ------------------------------------------------------------------------------------------------ (b) the entries
def test_entries_refuse_bad_arguments():
    from randlanet import _hip as H
    lib = H.lib()
    c = ti.case("13x11x9")
    states, cloud = ti.twin("13x11x9")
    nx, ny, nz = c.dims
    V = nx * ny * nz
    cam = c.camera
    with torch.cuda.device(_dev()):
        tsdf = torch.from_numpy(np.array(states[0][0])).to(_dev())
        weight = torch.from_numpy(np.array(states[0][1])).to(_dev())
        depth = torch.from_numpy(np.array(c.frames[1][0])).to(_dev())
        count = torch.zeros(1, dtype=torch.int64, device=_dev())
        need = lib.rl_tsdf_workspace_bytes(V)
        ws = torch.zeros(need + 256, dtype=torch.uint8, device=_dev())
        origin = (ctypes.c_float * 3)(*[float(F32(o)) for o in c.origin])
        rt = (ctypes.c_float * 12)(*[float(x) for x in _T().world_to_camera(c.frames[1][1])])
        voxel = float(F32(c.voxel))
        trunc = float(F32(4) * F32(c.voxel))
        nan = float("nan")
        good = [tsdf.data_ptr(), weight.data_ptr(), nx, ny, nz, origin, voxel, trunc, 64, depth.data_ptr(), cam.width, cam.height,
                float(cam.fx), float(cam.fy), float(cam.ppx), float(cam.ppy), float(cam.depth_scale), 0.05, 0.6, rt, None]
        bad = [(0, None), (1, None), (0, tsdf.data_ptr() + 2), (2, 0), (4, -1), (5, None), (6, 0.0), (6, nan), (7, 0.0), (7, nan),
               (8, 0), (8, 65536), (9, None), (9, depth.data_ptr() + 1), (10, 0), (11, 0), (10, 2 ** 24), (12, 0.0), (13, nan),
               (14, nan), (16, 0.0), (17, 0.6), (18, nan), (19, None)]
        torch.cuda.synchronize()
        before = lib.rl_launch_count()
        for pos, value in bad:
            args = list(good)
            args[pos] = value
            assert lib.rl_tsdf_integrate(*args) == H.ERR_ARGS, (pos, value)
            assert b"rl_tsdf_integrate" in lib.rl_last_error()
        assert lib.rl_launch_count() == before
        assert lib.rl_tsdf_integrate(*good) == 0 and lib.rl_launch_count() == before + 1
        ti.assert_same_state((tsdf, weight), states[1])
        # count and points
        good_c = [tsdf.data_ptr(), weight.data_ptr(), nx, ny, nz, origin, voxel, 1, count.data_ptr(), ws.data_ptr(), need, None]
        for pos, value in [(0, None), (1, weight.data_ptr() + 1), (3, 0), (5, None), (6, -1.0), (7, 0), (7, 65536), (8, None), (9, None),
                           (9, ws.data_ptr() + 8), (10, need - 1), (10, 0)]:
            args = list(good_c)
            args[pos] = value
            assert lib.rl_tsdf_count(*args) == H.ERR_ARGS, (pos, value)
            assert b"rl_tsdf_count" in lib.rl_last_error()
        assert lib.rl_launch_count() == before + 1
        assert lib.rl_tsdf_count(*good_c) == 0 and lib.rl_launch_count() == before + 3
        M = int(count.item())
        assert M == cloud.edge.shape[0]
        xyz = torch.full((M + 2, 3), 9.0, dtype=torch.float32, device=_dev())
        edge = torch.full((M + 2,), -9, dtype=torch.int64, device=_dev())
        good_p = [tsdf.data_ptr(), weight.data_ptr(), nx, ny, nz, origin, voxel, 1, M, xyz.data_ptr(), edge.data_ptr(), M, ws.data_ptr(),
                  need, None]
        for pos, value in [(0, None), (8, 0), (8, M + 1), (8, 3 * V + 1), (9, None), (10, None), (10, edge.data_ptr() + 4), (11, M - 1),
                           (12, None), (13, need - 1), (7, 0), (2, 0)]:
            args = list(good_p)
            args[pos] = value
            assert lib.rl_tsdf_points(*args) == H.ERR_ARGS, (pos, value)
            assert b"rl_tsdf_points" in lib.rl_last_error()
        assert lib.rl_launch_count() == before + 3
        assert lib.rl_tsdf_points(*good_p) == 0 and lib.rl_launch_count() == before + 4
        assert lib.rl_last_kernel() == b"ts_write"
        ti.assert_same_cloud((xyz[:M], edge[:M]), cloud)
        assert bool((xyz[M:] == 9.0).all()) and bool((edge[M:] == -9).all())      # exactly M rows were written


def test_workspace_bytes():
    from randlanet import _hip
    from randlanet import _ops as ops
    lib = _hip.lib()
    for V in (-1, 0, 2 ** 31, 2 ** 40):
        assert lib.rl_tsdf_workspace_bytes(V) == 0, V
    last = 0
    for V in (1, 1023, 1024, 1025, 128 * 128 * 80, 256 ** 3, 2 ** 31 - 1):
        n = lib.rl_tsdf_workspace_bytes(V)
        chunks = -(-V // 1024)
        assert 4 * chunks <= n < 4 * chunks + 256 and n % 256 == 0 and n >= last, V        # a count per chunk
        last = n
    with torch.cuda.device(_dev()):
        assert ops.tsdf_workspace(_dev(), 1025).numel() == 256


# ------------------------------------------------------------------------------------------------ (c) the camera loop
def _model(use_gpu=True, weights=None):
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    return Model(RandLANetSettings(n_classes=4, n_points=512, n_neighbors=8, layer_sizes=[8, 16, 32, 32], n_features=0),
                 weights=weights, use_gpu=use_gpu)


@pytest.fixture(scope="module")
def models():
    gpu = _model()
    assert gpu.device.type == "cuda"
    weights = {k: v.detach().cpu().clone() for k, v in gpu.module.state_dict().items()}
    return gpu, _model(use_gpu=False, weights=weights)


PLACEMENT_TOL = 1e-4          # confidences of the two placements: tests/test_scene_gpu.py::test_predict_scene_gpu_matches_cpu_model


@pytest.mark.parametrize("tracked", (False, True))
def test_depth_fusion_equals_the_cpu_placed_copy(models, tracked):
    """The same calls on a GPU model and on a CPU-placed copy: poses, fitness and rmse are equal (the ICP is bit-equal), the
    surface is equal bit for bit, and predict() is predict_scene on the extracted tensor by hand."""
    T = _T()
    from randlanet.utils.depth import TemporalFilter
    from randlanet.utils.registration import IcpSettings
    gpu_model, cpu_model = models
    c = ti.sphere_case(ground=True, poses=ti.TRACK_POSES) if tracked else ti.case("sphere")
    kw = dict(icp=IcpSettings(max_distance=0.02), min_weight=1) if tracked else {}
    fusions = [T.DepthFusion(m, c.camera, ti.volume(c, "cpu"), temporal=TemporalFilter(), z_range=c.z_range, **kw)
               for m in (gpu_model, cpu_model)]
    assert fusions[0].volume.tsdf.is_cuda and isinstance(fusions[1].volume.tsdf, np.ndarray)
    for k, (depth, pose) in enumerate(c.frames):
        got, want = (f.add(np.array(depth), None if tracked else pose) for f in fusions)
        assert got.status == want.status and got.integrated == want.integrated and got.status != "degenerate", k
        assert np.array_equal(got.transformation, want.transformation), k
        assert got.fitness == want.fitness and got.inlier_rmse == want.inlier_rmse, k
        ti.assert_same_state((fusions[0].volume.tsdf, fusions[0].volume.weight), (fusions[1].volume.tsdf, fusions[1].volume.weight), k)
        assert np.array_equal(_np(fusions[0].temporal.state), fusions[1].temporal.state)
    surf, host = fusions[0].surface(), fusions[1].surface()
    assert surf.xyz.is_cuda and surf.edge.is_cuda and surf.xyz.shape[0] > 300
    ti.assert_same_cloud(surf, host)
    assert np.array_equal(fusions[0].transformations, fusions[1].transformations)
    vote = dict(batch_size=2, seed=2, pad_small_scenes=True)
    np.random.seed(5)
    got = fusions[0].predict(**vote)
    np.random.seed(5)
    by_hand = gpu_model.predict_scene(fusions[0].volume.extract(fusions[0].min_weight).xyz, None, **vote)
    assert isinstance(got, T.FusedPrediction) and all(isinstance(a, np.ndarray) for a in got)
    assert np.array_equal(got.confidences.view(np.uint32), by_hand.view(np.uint32))
    ti.assert_same_cloud((got.xyz, got.edge), host)
    np.random.seed(5)
    placed = fusions[1].predict(**vote)
    print("largest difference between the placements:", np.abs(got.confidences - placed.confidences).max())
    assert np.abs(got.confidences - placed.confidences).max() < PLACEMENT_TOL
    fusions[0].reset()
    assert fusions[0].volume.tsdf.is_cuda and bool((fusions[0].volume.weight == 0).all()) and fusions[0].temporal.state is None
    with pytest.raises(ValueError, match="the surface is empty"):
        fusions[0].predict()
    with pytest.raises(ValueError, match="no pixel inside z_range"):
        fusions[0].add(np.zeros(ti.LARGE, np.uint16))
