"""Depth frames to points on the host: the numpy twin (utils/depth.py) against the scalar yardstick of tests/depth_inputs.py,
bit for bit, and against an fp64 evaluation; the reference's points[filter] semantics; the strict bounds; the stride; the
temporal filter branch by branch; the refusals; and predict_depth of a CPU-placed Model."""
import numpy as np
import pytest
import torch

import depth_inputs as di

F32 = np.float32


def _D():
    from randlanet.utils import depth
    return depth


# ------------------------------------------------------------------------------------------------ 1. twin against yardsticks
@pytest.mark.parametrize("name", di.SCALAR)
def test_twin_equals_the_scalar_loop(name):
    depth, cam, z_range, stride = di.case(name)
    xyz, pixel = di.yardstick(depth, cam, z_range, stride)
    got = di.twin(name)
    di.assert_same(got, _D().DepthCloud(xyz, pixel), name)
    assert got.xyz.flags.c_contiguous and (np.diff(got.pixel) > 0).all()
    if name in ("5x67-random", "5x67-random-coeffs"):
        assert 100 < got.pixel.shape[0] < 5 * 67 - 20
    # the public function on the host path is the twin
    di.assert_same(_D().deproject(depth, cam, z_range, stride, device="cpu"), got, name)


def test_coefficients_change_the_points():
    a, b = di.twin("5x67-random"), di.twin("5x67-random-coeffs")
    same = np.intersect1d(a.pixel, b.pixel)
    assert same.size > 50
    xa, xb = a.xyz[np.isin(a.pixel, same)], b.xyz[np.isin(b.pixel, same)]
    assert (xa[:, :2] != xb[:, :2]).any()


def test_twin_against_fp64():
    """x and y of every kept point within 4 * 2^-24 relative of the fp64 evaluation from the same float32 intrinsics: four
    roundings (subtract, divide, z, product), the operands exact."""
    depth, cam, z_range, _ = di.case("5x67-random")
    got = di.twin("5x67-random")
    W = depth.shape[1]
    v, u = (got.pixel // W).astype(np.float64), (got.pixel % W).astype(np.float64)
    z = depth.reshape(-1)[got.pixel].astype(np.float64) * np.float64(cam.depth_scale)
    x = (u - np.float64(cam.ppx)) / np.float64(cam.fx) * z
    y = (v - np.float64(cam.ppy)) / np.float64(cam.fy) * z
    ex = np.abs(got.xyz[:, 0] - x) / np.abs(x)
    ey = np.abs(got.xyz[:, 1] - y) / np.abs(y)
    print("worst relative error in units of 2^-24:", max(ex.max(), ey.max()) * 2.0 ** 24)
    assert max(ex.max(), ey.max()) <= 4 * 2.0 ** -24
    assert (np.abs(got.xyz[:, 2] - z) <= np.abs(z) * 2.0 ** -24).all()


def test_reference_semantics_points_of_filter():
    """xyz is the full per-pixel deprojection indexed by the reference's mask: points[filter]."""
    depth, cam, _, _ = di.case("5x67-random")
    H, W = depth.shape
    v, u = np.mgrid[0:H, 0:W]
    z = depth.astype(F32) * cam.depth_scale
    x = (u.astype(F32) - cam.ppx) / cam.fx * z
    y = (v.astype(F32) - cam.ppy) / cam.fy * z
    points = np.stack((x, y, z), axis=-1).reshape(-1, 3)
    zz = points[:, 2]
    keep = (F32(0.05) < zz) & (zz < F32(0.6)) & (depth.reshape(-1) != 0)
    got = di.twin("5x67-random")
    assert np.array_equal(got.xyz.view(np.uint32), points[keep].view(np.uint32))
    assert np.array_equal(got.pixel, np.flatnonzero(keep))


def test_bounds_are_strict():
    D = _D()
    cam = di.camera(1, 4)
    depth = np.array([[200, 201, 2399, 2400]], np.uint16)
    z_lo, z_hi = F32(200) * cam.depth_scale, F32(2400) * cam.depth_scale
    got = D.deproject_host(depth, cam, (z_lo, z_hi))
    assert np.array_equal(got.pixel, [1, 2])
    assert np.array_equal(D.deproject_host(depth, cam, (F32(199) * cam.depth_scale, z_hi)).pixel, [0, 1, 2])
    assert np.array_equal(D.deproject_host(depth, cam, (z_lo, F32(2401) * cam.depth_scale)).pixel, [1, 2, 3])
    # a raw 0 is no point even inside the range
    assert np.array_equal(D.deproject_host(np.array([[0, 5, 0, 7]], np.uint16), cam, (-1.0, 1.0)).pixel, [1, 3])
    empty = D.deproject_host(np.zeros((1, 4), np.uint16), cam)
    assert empty.xyz.shape == (0, 3) and empty.xyz.dtype == F32 and empty.pixel.shape == (0,) and empty.pixel.dtype == np.int32


@pytest.mark.parametrize("stride", [2, 3])
def test_stride_on_odd_dimensions(stride):
    depth, cam, z_range, _ = di.case("5x67-random")
    whole = di.twin("5x67-random")
    got = di.twin(f"5x67-random-stride{stride}")
    v, u = whole.pixel // 67, whole.pixel % 67
    part = (v % stride == 0) & (u % stride == 0)
    assert 0 < part.sum() < whole.pixel.shape[0]
    di.assert_same(got, _D().DepthCloud(np.ascontiguousarray(whole.xyz[part]), whole.pixel[part]))


# ------------------------------------------------------------------------------------------------ 2. the temporal filter
def test_temporal_filter_branch_by_branch():
    D = _D()
    frames = di.temporal_frames()
    want = di.temporal_yardstick(frames)
    filt = D.TemporalFilter(di.ALPHA, di.DELTA)
    assert filt.state is None and filt.one_minus_alpha == F32(1) - F32(di.ALPHA)
    outs = []
    for k, frame in enumerate(frames):
        out = filt.process(frame, device="cpu")
        assert out.dtype == np.uint16 and out.shape == di.T_SHAPE
        assert np.array_equal(out, want[k][0]), k
        assert isinstance(filt.state, np.ndarray) and np.array_equal(filt.state, want[k][1]), k
        outs.append(out.reshape(-1))
    o = np.array(outs)
    assert (o[:, di.T_FIRST] == 1000).all()
    assert o[:, di.T_HOLE].tolist() == [1000, 0, 1013, 0, 0]            # 0.33 * 1040 + 0.67 * 1000 + 0.5 = 1013.7
    assert filt.state.reshape(-1)[di.T_HOLE] == 1013                    # the holes since kept it
    assert o[1, di.T_BELOW] == 1033                                     # 0.33 * 1099 + 0.67 * 1000 + 0.5 = 1033.17
    assert o[:, di.T_AT].tolist() == [1000, 1100, 1000, 1100, 1200]
    assert o[1, di.T_HALF] == 1002
    assert 65500 < o[1, di.T_TOP] <= 65535 and (o[:, di.T_TOP] <= 65535).all()
    assert (o[:, di.T_NEVER] == 0).all() and filt.state.reshape(-1)[di.T_NEVER] == 0
    # every branch was taken by the other pixels too
    c, p = frames[2].astype(int), want[1][1].astype(int)
    live = (c != 0) & (p != 0)
    assert (c == 0).any() and (p == 0).any() and (live & (abs(c - p) < di.DELTA)).any() and (live & (abs(c - p) >= di.DELTA)).any()
    # reset(): the next frame is a first sight everywhere
    filt.reset()
    assert filt.state is None
    assert np.array_equal(filt.process(frames[1], device="cpu"), frames[1])
    # a frame of another shape is refused, and the state stays
    before = filt.state.copy()
    with pytest.raises(ValueError, match=r"depth has shape \(3, 66\), the filter's state \(3, 67\)"):
        filt.process(np.zeros((3, 66), np.uint16), device="cpu")
    assert np.array_equal(filt.state, before)
    filt.reset()
    assert filt.process(np.zeros((3, 66), np.uint16), device="cpu").shape == (3, 66)


def test_depth_points_is_filter_then_deproject():
    D = _D()
    frames = di.temporal_frames()
    cam = di.camera(*di.T_SHAPE)
    a, b = D.TemporalFilter(), D.TemporalFilter()
    for frame in frames:
        got = D.depth_points(frame, cam, a, stride=1, device="cpu")
        want = D.deproject_host(b.process(frame, device="cpu"), cam)
        di.assert_same(got, want)
        assert np.array_equal(a.state, b.state)
    assert got.pixel.shape[0] > 50


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals():
    D = _D()
    cam = di.camera(3, 67)
    good = np.zeros((3, 67), np.uint16)
    for bad, match in ((good.astype(np.int16), "dtype int16, expected uint16"), (good.astype(np.float32), "dtype float32"),
                       (good[0], r"shape \(67,\), expected \(H, W\)"), (good[None], r"expected \(H, W\)"),
                       (good[:, :66], r"shape \(3, 66\), expected \(3, 67\)"), (good.T, r"expected \(3, 67\)"),
                       (np.zeros((3, 134), np.uint16)[:, ::2], "C-contiguous"), ([[1, 2]], "numpy array or a torch tensor")):
        for fn in (D.deproject_host, lambda d, c: D.deproject(d, c, device="cpu"), lambda d, c: D.depth_points(d, c, device="cpu")):
            with pytest.raises(ValueError, match=match):
                fn(bad, cam)
    with pytest.raises(ValueError, match="dtype int16"):
        D.deproject(torch.zeros((3, 67), dtype=torch.int16), cam, device="cpu")
    with pytest.raises(ValueError, match="camera="):
        D.deproject_host(good, (67, 3, 1.0, 1.0, 0.0, 0.0, 1.0, None))
    for stride in (0, -1, 1.5, "2", True, None):
        with pytest.raises(ValueError, match="stride="):
            D.deproject_host(good, cam, stride=stride)
    for z_range in ((0.6, 0.05), (0.3, 0.3), (float("nan"), 1.0), (0.1, float("nan")), (0.1,), 0.5, "ab", (0.1, 0.2, 0.3)):
        with pytest.raises(ValueError, match="z_range="):
            D.deproject_host(good, cam, z_range)
    with pytest.raises(ValueError, match="z_range="):          # equal once rounded to float32
        D.deproject_host(good, cam, (0.1, 0.1 + 1e-12))
    for name in ("fx", "fy", "depth_scale"):
        for value in (0.0, -1.0, float("inf"), float("nan"), 1e-60, None, "1"):
            kw = dict(width=67, height=3, fx=1.0, fy=1.0, ppx=0.0, ppy=0.0, depth_scale=0.001)
            kw[name] = value
            with pytest.raises(ValueError, match=f"{name}="):
                D.DepthCamera(**kw)
    for name in ("ppx", "ppy"):
        with pytest.raises(ValueError, match=f"{name}="):
            D.DepthCamera(**{**dict(width=67, height=3, fx=1.0, fy=1.0, ppx=0.0, ppy=0.0, depth_scale=0.001), name: float("inf")})
    for w, h in ((0, 3), (3, -1), (2.5, 3), (2 ** 16, 2 ** 15), (2 ** 31, 1)):           # H * W >= 2^31
        with pytest.raises(ValueError, match="width=|height="):
            D.DepthCamera(w, h, 1.0, 1.0, 0.0, 0.0, 0.001)
    assert D.DepthCamera(2 ** 16, 2 ** 15 - 1, 1.0, 1.0, 0.0, 0.0, 0.001).width == 2 ** 16
    for coeffs in ((1, 2, 3, 4), (1, 2, 3, 4, float("nan")), "abcde", 1.0):
        with pytest.raises(ValueError, match="coeffs"):
            D.DepthCamera(67, 3, 1.0, 1.0, 0.0, 0.0, 0.001, coeffs)
    for alpha in (0.0, -0.1, 1.0001, float("nan"), 1e-60, None, "a"):
        with pytest.raises(ValueError, match="alpha="):
            D.TemporalFilter(alpha=alpha)
    assert D.TemporalFilter(alpha=1.0).one_minus_alpha == 0
    for delta in (0, -1, 65536, 1.5, None):
        with pytest.raises(ValueError, match="delta="):
            D.TemporalFilter(delta=delta)
    assert D.TemporalFilter(delta=1).delta == 1 and D.TemporalFilter(delta=65535).delta == 65535
    with pytest.raises(ValueError, match="temporal="):
        D.depth_points(good, cam, temporal=0.33, device="cpu")


def test_camera_is_immutable_and_float32():
    cam = di.camera(3, 67, coeffs=True)
    assert all(type(getattr(cam, n)) is np.float32 for n in ("fx", "fy", "ppx", "ppy", "depth_scale"))
    assert cam.fx == F32(730.5) and cam.ppx == F32(67 / 2 - 0.2) and cam.depth_scale == F32(0.00025)
    assert len(cam.coeffs) == 5 and all(type(c) is np.float32 for c in cam.coeffs) and cam.coeffs[0] == F32(0.11)
    assert cam.width == 67 and cam.height == 3 and di.camera(3, 67).coeffs is None
    with pytest.raises(AttributeError):
        cam.fx = 1.0
    with pytest.raises(AttributeError):
        cam.extra = 1.0


# ------------------------------------------------------------------------------------------------ 4. a CPU-placed Model
@pytest.fixture(scope="module")
def cpu_model():
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    return Model(RandLANetSettings(n_classes=4, n_points=512, n_neighbors=8, layer_sizes=[8, 16, 32, 32]), use_gpu=False)


def test_predict_depth_on_a_cpu_placed_model(cpu_model):
    D = _D()
    depth, cam = di.plane_frame()
    want_cloud = D.deproject_host(depth, cam, stride=2)
    assert 2048 < want_cloud.pixel.shape[0] < 48 * 64
    np.random.seed(3)
    got = cpu_model.predict_depth(depth, cam, stride=2)
    np.random.seed(3)
    want = cpu_model.predict(want_cloud.xyz)
    assert isinstance(got, D.DepthPrediction) and got.confidences.shape == (4, want_cloud.pixel.shape[0])
    assert np.array_equal(got.confidences.view(np.uint32), want.view(np.uint32))
    di.assert_same((got.xyz, got.pixel), want_cloud)
    # fewer points than n_points, and the filter's state carried by the caller's object
    filt, twin_filt = D.TemporalFilter(), D.TemporalFilter()
    small = D.deproject_host(twin_filt.process(depth, device="cpu"), cam, (0.2, 0.24))
    assert 100 < small.pixel.shape[0] < 512
    np.random.seed(3)
    got_small = cpu_model.predict_depth(depth, cam, temporal=filt, z_range=(0.2, 0.24))
    np.random.seed(3)
    assert np.array_equal(got_small.confidences.view(np.uint32), cpu_model.predict(small.xyz).view(np.uint32))
    assert np.array_equal(filt.state, twin_filt.state)
    # image(): column j at pixel[j]
    img = got.image(96, 128, fill=-1.0)
    assert img.shape == (4, 96, 128) and img.dtype == F32
    flat = img.reshape(4, -1)
    assert np.array_equal(flat[:, got.pixel], got.confidences)
    rest = np.ones(96 * 128, bool)
    rest[got.pixel] = False
    assert (flat[:, rest] == -1.0).all() and (got.image(96, 128).reshape(4, -1)[:, rest] == 0.0).all()
    with pytest.raises(ValueError, match="pixel indices outside"):
        got.image(10, 10)


def test_predict_depth_refusals(cpu_model):
    depth, cam = di.plane_frame()
    with pytest.raises(ValueError, match="predict_depth: no pixel inside z_range"):
        cpu_model.predict_depth(np.zeros((96, 128), np.uint16), cam)
    with pytest.raises(ValueError, match="predict_depth: no pixel inside z_range"):
        cpu_model.predict_depth(depth, cam, z_range=(5.0, 6.0))
    with pytest.raises(ValueError, match="stride="):
        cpu_model.predict_depth(depth, cam, stride=0)
    with pytest.raises(ValueError, match=r"expected \(96, 128\)"):
        cpu_model.predict_depth(depth[:90], cam)
    with pytest.raises(AssertionError, match="at least"):            # below the network's minimum: predict's own assertion
        cpu_model.predict_depth(depth, cam, z_range=(0.2, 0.206), prepostprocess=False)


def test_a_cpu_placed_model_refuses_device_clouds(cpu_model):
    """(Distinct points and a bound on the passes: where the tensor is not refused the call ends, and the test fails at once.)"""
    xyz = torch.from_numpy(np.random.RandomState(2).uniform(0, 1, (600, 3)).astype(F32))
    with pytest.raises(ValueError, match="placed on the CPU"):
        cpu_model.predict_scene(xyz, batch_size=2, max_passes=2)
    with pytest.raises(ValueError, match="placed on the CPU"):
        cpu_model.predict_keypoints(xyz, radius=0.1, batch_size=2, max_passes=2)
