"""Depth frames to points on the MI355X: csrc/depth.hip against the numpy twin (utils/depth.py) on every case of
tests/depth_inputs.py, bit for bit - the cloud, M, the filtered frame and the resident state; frames that are only 2-byte
aligned; the entry's refusals and workspace; Model.predict_depth against predict on the twin's cloud; and device clouds into
predict_scene / predict_keypoints."""
import numpy as np
import pytest
import torch

import depth_inputs as di

pytestmark = pytest.mark.gpu
F32 = np.float32


def _dev():
    return torch.device("cuda", 0)


def _D():
    from randlanet.utils import depth
    return depth


def _np(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ (a) kernels against twin
@pytest.mark.parametrize("name", di.CASES)
def test_device_equals_the_twin(name):
    from randlanet import _hip
    depth, cam, z_range, stride = di.case(name)
    want = di.twin(name)
    got = _D().deproject(np.array(depth), cam, z_range, stride, device=_dev())
    assert _hip.lib().rl_last_kernel() == b"dp_write"
    assert torch.is_tensor(got.xyz) and got.xyz.is_cuda and got.pixel.is_cuda and got.xyz.is_contiguous()
    assert got.xyz.shape[0] == want.pixel.shape[0]            # M
    di.assert_same(got, want, name)
    if name.endswith("-zero"):
        assert got.xyz.shape == (0, 3) and got.pixel.shape == (0,)
    if name == "768x1024-random":
        assert 300000 < want.pixel.shape[0] < 450000


def test_default_device_and_device_input():
    depth, cam, z_range, stride = di.case("3x67-random")
    want = di.twin("3x67-random")
    got = _D().deproject(np.array(depth), cam)                 # device=None: a GPU is available
    assert got.xyz.is_cuda
    di.assert_same(got, want)
    frame = torch.from_numpy(np.array(depth)).to(_dev())
    got = _D().deproject(frame, cam)                           # a device tensor stays where it is
    assert got.xyz.is_cuda
    di.assert_same(got, want)
    di.assert_same(_D().deproject(frame, cam, device="cpu"), want)
    assert isinstance(_D().deproject(frame, cam, device="cpu").xyz, np.ndarray)


@pytest.mark.parametrize("shape", [(3, 67), (5, 1027)])
def test_a_frame_that_is_only_2_byte_aligned(shape):
    """Frame 1 of a (2, H, W) tensor with odd H * W: the same cloud as the frame uploaded on its own; so for the temporal
    filter, whose state and output are aligned differently from the frame."""
    from randlanet import _ops as ops
    D = _D()
    H, W = shape
    cam = di.camera(H, W)
    both = np.stack([di.contents(H, W, "random", 5), di.contents(H, W, "random", 6)])
    batch = torch.from_numpy(both).to(_dev())
    frame = batch[1]
    assert frame.is_contiguous() and frame.data_ptr() % 16 == 2 * ((H * W) % 8) != 0
    want = D.deproject_host(both[1], cam)
    di.assert_same(D.deproject(frame, cam), want)
    di.assert_same(D.deproject(torch.from_numpy(both[1]).to(_dev()), cam), want)
    assert np.array_equal(_np(batch), both)                    # nothing around the frame was written
    # the filter: two frames through a resident state
    host, filt = D.TemporalFilter(), D.TemporalFilter()
    for k in (0, 1):
        w_out = host.process(both[k], device="cpu")
        with torch.cuda.device(_dev()):
            state = filt._device_state((H, W), _dev())
            xyz, pixel, out = ops.depth_points(batch[k], cam, F32(0.05), F32(0.6), 1, state,
                                               (filt.alpha, filt.one_minus_alpha, filt.delta), want_filtered=True)
        assert np.array_equal(_np(out), w_out) and np.array_equal(_np(filt.state), host.state)
        di.assert_same((xyz, pixel), D.deproject_host(w_out, cam))
    # a misaligned state and output against an aligned frame
    pad = torch.zeros(2 * H * W + 1, dtype=torch.int16, device=_dev()).view(torch.uint16)
    state = pad[1:1 + H * W].view(H, W)
    host.reset()
    for k in (0, 1):
        w_out = host.process(both[k], device="cpu")
        with torch.cuda.device(_dev()):
            got = ops.temporal_filter(torch.from_numpy(both[k]).to(_dev()), state, host.alpha, host.one_minus_alpha, host.delta)
        assert np.array_equal(_np(got), w_out) and np.array_equal(_np(state), host.state)
    around = _np(pad)
    assert around[0] == 0 and not around[1 + H * W:].any()                   # nothing around the state was written


# ------------------------------------------------------------------------------------------------ (b) the temporal sequence
def test_temporal_sequence_with_a_resident_state():
    from randlanet import _hip
    D = _D()
    frames = di.temporal_frames()
    want = di.temporal_yardstick(frames)
    cam = di.camera(*di.T_SHAPE)
    alone, fused, host, second = D.TemporalFilter(), D.TemporalFilter(), D.TemporalFilter(), D.TemporalFilter()
    for k, frame in enumerate(frames):
        out = alone.process(np.array(frame), device=_dev())
        assert _hip.lib().rl_last_kernel() == b"dp_write"
        assert torch.is_tensor(out) and out.is_cuda and out.dtype == torch.uint16
        assert np.array_equal(_np(out), want[k][0]), k
        assert alone.state.is_cuda and np.array_equal(_np(alone.state), want[k][1]), k
        got = D.depth_points(np.array(frame), cam, fused, device=_dev())          # the fused entry: filter, then points
        di.assert_same(got, D.depth_points(frame, cam, host, device="cpu"), k)
        assert np.array_equal(_np(fused.state), want[k][1]) and np.array_equal(host.state, want[k][1]), k
    # a second filter does not see the first one's state
    assert second.state is None
    assert np.array_equal(_np(second.process(np.array(frames[1]), device=_dev())), frames[1])
    assert np.array_equal(_np(alone.state), want[-1][1])
    alone.reset()
    assert np.array_equal(_np(alone.process(np.array(frames[2]), device=_dev())), frames[2])
    with pytest.raises(ValueError, match="the filter's state"):
        alone.process(np.zeros((3, 66), np.uint16), device=_dev())
    # a state begun on the host goes on on the device
    moved = D.TemporalFilter()
    moved.process(frames[0], device="cpu")
    assert np.array_equal(_np(moved.process(np.array(frames[1]), device=_dev())), want[1][0])


def test_temporal_filter_on_a_large_frame():
    D = _D()
    rs = np.random.RandomState(8)
    a = rs.randint(0, 3000, (257, 1031)).astype(np.uint16)
    b = np.clip(a.astype(int) + rs.randint(-150, 151, a.shape), 0, 65535).astype(np.uint16)
    b[rs.uniform(size=a.shape) < 0.1] = 0
    cam = di.camera(257, 1031, coeffs=True)
    dev, host = D.TemporalFilter(0.4, 120), D.TemporalFilter(0.4, 120)
    for frame in (a, b, a):
        di.assert_same(D.depth_points(frame, cam, dev, stride=2, device=_dev()), D.depth_points(frame, cam, host, stride=2, device="cpu"))
        assert np.array_equal(_np(dev.state), host.state)


# ------------------------------------------------------------------------------------------------ (c) the entry
def test_entry_refuses_bad_arguments():
    from randlanet import _hip as H
    lib = H.lib()
    import ctypes
    with torch.cuda.device(_dev()):
        Hh, W = 3, 67
        P = Hh * W
        depth = torch.from_numpy(np.array(di.case("3x67-random")[0])).to(_dev())
        state = torch.zeros((Hh, W), dtype=torch.int16, device=_dev()).view(torch.uint16)
        out = torch.zeros((Hh, W), dtype=torch.int16, device=_dev()).view(torch.uint16)
        xyz = torch.zeros((P, 3), dtype=torch.float32, device=_dev())
        pixel = torch.zeros(P, dtype=torch.int32, device=_dev())
        count = torch.zeros(1, dtype=torch.int64, device=_dev())
        need = lib.rl_depth_workspace_bytes(P)
        ws = torch.zeros(need + 256, dtype=torch.uint8, device=_dev())
        coeffs = (ctypes.c_float * 5)(*di.COEFFS)
        bad_coeffs = (ctypes.c_float * 5)(0.1, float("nan"), 0.0, 0.0, 0.0)
        cam = di.camera(Hh, W)
        oma = float(F32(1) - F32(0.33))
        good = [depth.data_ptr(), state.data_ptr(), out.data_ptr(), W, Hh, 1, float(cam.fx), float(cam.fy), float(cam.ppx),
                float(cam.ppy), float(cam.depth_scale), ctypes.addressof(coeffs), float(F32(0.33)), oma, 100, 0.05, 0.6,
                xyz.data_ptr(), pixel.data_ptr(), count.data_ptr(), ws.data_ptr(), need, None]
        nan, inf = float("nan"), float("inf")
        bad = [(0, None), (0, depth.data_ptr() + 1), (1, state.data_ptr() + 1), (2, out.data_ptr() + 1),
               (3, 0), (3, -1), (4, 0), (3, 2 ** 31 - 1), (5, 0), (5, -2),
               (6, 0.0), (6, -1.0), (6, nan), (6, inf), (7, 0.0), (7, nan), (7, inf), (8, nan), (8, inf), (9, nan), (9, -inf),
               (10, 0.0), (10, -0.001), (10, nan), (10, inf), (11, ctypes.addressof(bad_coeffs)),
               (12, 0.0), (12, 1.5), (12, nan), (13, -0.1), (13, 1.0), (13, nan), (14, 0), (14, 65536), (14, -5),
               (15, 0.6), (15, 0.7), (15, nan), (16, nan), (17, None), (18, None), (19, None),
               (20, None), (20, ws.data_ptr() + 8), (21, need - 1), (21, 0)]
        torch.cuda.synchronize()
        before = lib.rl_launch_count()
        for pos, value in bad:
            args = list(good)
            args[pos] = value
            assert lib.rl_depth_points(*args) == H.ERR_ARGS, (pos, value)
            assert b"rl_depth_points" in lib.rl_last_error()
        # no state and no outputs for the points: nothing to do
        args = list(good)
        args[1] = args[17] = args[18] = args[19] = None
        assert lib.rl_depth_points(*args) == H.ERR_ARGS
        assert lib.rl_launch_count() == before
        assert lib.rl_depth_points(*good) == 0 and lib.rl_launch_count() == before + 3
        assert lib.rl_last_kernel() == b"dp_write"
        # the filter alone: one launch, and its parameters are not read without a state
        args = list(good)
        args[17] = args[18] = args[19] = args[20] = None
        args[21] = 0
        assert lib.rl_depth_points(*args) == 0 and lib.rl_launch_count() == before + 4
        args = list(good)
        args[1], args[12], args[13], args[14] = None, 0.0, 0.0, 0
        assert lib.rl_depth_points(*args) == 0 and lib.rl_launch_count() == before + 7
        torch.cuda.synchronize()
        want = _D().deproject_host(di.case("3x67-random")[0], di.camera(Hh, W, coeffs=True))
        M = int(count.item())
        di.assert_same((xyz[:M], pixel[:M]), want)
        assert np.array_equal(_np(out), di.case("3x67-random")[0])             # without a state the output is the frame


def test_workspace_bytes():
    from randlanet import _hip
    lib = _hip.lib()
    for P in (-1, 0, 2 ** 31, 2 ** 40):
        assert lib.rl_depth_workspace_bytes(P) == 0, P
    last = 0
    for P in (1, 8, 1017, 1018, 1024, 1025, 768 * 1024, 10 ** 7, 2 ** 31 - 1):
        n = lib.rl_depth_workspace_bytes(P)
        chunks = -(-P // 1024)
        assert n >= 4 * chunks and n % 256 == 0 and n >= last, P          # a count per chunk
        assert n <= 4 * (chunks + 1) + 256, P
        last = n


# ------------------------------------------------------------------------------------------------ (d) Model
def _model(use_gpu=True, weights=None):
    """The settings of tests/test_outliers_gpu.py's _model()."""
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    return Model(RandLANetSettings(n_classes=3, n_points=2048, n_neighbors=8, layer_sizes=[8, 16, 32, 32], n_features=0),
                 weights=weights, use_gpu=use_gpu)


@pytest.fixture(scope="module")
def gpu_model():
    model = _model()
    assert model.device.type == "cuda"
    return model


# confidences of the two placements: the bound tests/test_scene_gpu.py::test_predict_scene_gpu_matches_cpu_model (and the grid
# and padded-scene tests after it) holds the GPU- and the CPU-placed model to
PLACEMENT_TOL = 1e-4


@pytest.mark.parametrize("z_range,above", [((0.05, 0.6), True), ((0.2, 0.26), False)])
def test_predict_depth_equals_predict_on_the_twins_cloud(gpu_model, z_range, above):
    D = _D()
    depth, cam = di.plane_frame()
    twin = D.deproject_host(depth, cam, z_range)
    M = twin.pixel.shape[0]
    assert (M > 2048) == above and M > 512
    np.random.seed(3)
    got = gpu_model.predict_depth(np.array(depth), cam, z_range=z_range)
    state = np.random.get_state()[1].copy()
    np.random.seed(3)
    want = gpu_model.predict(twin.xyz)
    assert np.array_equal(np.random.get_state()[1], state)
    assert isinstance(got, D.DepthPrediction) and all(isinstance(a, np.ndarray) for a in got)
    assert got.confidences.shape == (3, M) and got.confidences.dtype == F32
    di.assert_same((got.xyz, got.pixel), twin)
    assert np.array_equal(got.confidences.view(np.uint32), want.view(np.uint32))
    weights = {k: v.detach().cpu().clone() for k, v in gpu_model.module.state_dict().items()}
    cpu_model = _model(use_gpu=False, weights=weights)
    np.random.seed(3)
    host = cpu_model.predict_depth(depth, cam, z_range=z_range)
    di.assert_same((host.xyz, host.pixel), twin)
    print("largest difference between the placements:", np.abs(got.confidences - host.confidences).max())
    assert np.abs(got.confidences - host.confidences).max() < PLACEMENT_TOL


def test_predict_depth_with_the_filter_and_refusals(gpu_model):
    D = _D()
    depth, cam = di.plane_frame()
    second = np.array(depth)
    second[10:40, 10:60] += 30
    dev, host = D.TemporalFilter(), D.TemporalFilter()
    for frame in (np.array(depth), second):
        np.random.seed(4)
        got = gpu_model.predict_depth(frame, cam, temporal=dev, stride=2, prepostprocess=False)
        twin = D.depth_points(frame, cam, host, stride=2, device="cpu")
        np.random.seed(4)
        want = gpu_model.predict(twin.xyz, prepostprocess=False)
        di.assert_same((got.xyz, got.pixel), twin)
        assert np.array_equal(got.confidences.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(_np(dev.state), host.state)
    with pytest.raises(ValueError, match="predict_depth: no pixel inside z_range"):
        gpu_model.predict_depth(np.zeros((96, 128), np.uint16), cam)
    with pytest.raises(ValueError, match=r"expected \(96, 128\)"):
        gpu_model.predict_depth(np.zeros((96, 127), np.uint16), cam)
    with pytest.raises(AssertionError, match="at least"):
        gpu_model.predict_depth(np.array(depth), cam, z_range=(0.2, 0.206), prepostprocess=False)


# ------------------------------------------------------------------------------------------------ (e) device clouds
KW = dict(votes=1, batch_size=2, seed=2)


def test_device_clouds_into_the_scene_path(gpu_model):
    D = _D()
    depth, cam = di.plane_frame()
    cloud = D.depth_points(np.array(depth), cam, device=gpu_model.device)
    xyz_t = cloud.xyz
    xyz = _np(xyz_t)
    assert xyz_t.is_cuda and xyz.shape[0] > 2048
    for kw in (dict(return_counts=True), dict(return_counts=True, grid=0.0015), dict(outliers=(8, 2.0), return_outliers=True)):
        np.random.seed(5)
        got = gpu_model.predict_scene(xyz_t, **kw, **KW)
        np.random.seed(5)
        want = gpu_model.predict_scene(xyz, **kw, **KW)
        assert all(np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
                   for a, b in zip(got, want)), kw
    for kw in (dict(outliers=(8, 2.0)), dict(grid=0.0015)):
        kw = dict(radius=0.02, min_score=0.0, ignore_classes=(), **kw)
        np.random.seed(5)
        got = gpu_model.predict_keypoints(xyz_t, **kw, **KW)
        np.random.seed(5)
        want = gpu_model.predict_keypoints(xyz, **kw, **KW)
        assert got.index.shape[0] >= 1
        assert all(a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want)), kw
    assert np.array_equal(_np(xyz_t), xyz)                     # the caller's tensor is not written
    # refusals
    for fn in (gpu_model.predict_scene, lambda *a, **k: gpu_model.predict_keypoints(*a, radius=0.02, **k)):
        with pytest.raises(ValueError, match="xyz is a tensor on cpu"):
            fn(xyz_t.cpu(), **KW)
        with pytest.raises(ValueError, match="torch.float64 tensor, expected torch.float32"):
            fn(xyz_t.double(), **KW)
        with pytest.raises(ValueError, match="features must be None"):
            fn(xyz_t, np.zeros((xyz.shape[0], 1), F32), **KW)
        bad = xyz_t.clone()
        bad[7, 1] = float("nan")
        with pytest.raises(ValueError, match="non-finite coordinates"):
            fn(bad, **KW)
