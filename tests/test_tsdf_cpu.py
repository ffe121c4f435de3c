"""TSDF fusion on the host: the numpy twin (utils/tsdf.py) against the scalar restatements of tests/tsdf_inputs.py, bit for
bit; the designed contents - frustum, borders, truncation, saturation, planted crossings -; the geometry of a fused sphere; the
refusals; DepthFusion on a CPU-placed Model, with given poses and tracked; and the library's host-side refusals."""
import ctypes

import numpy as np
import pytest
import torch

import tsdf_inputs as ti

F32 = np.float32


def _T():
    from randlanet.utils import tsdf
    return tsdf


# ------------------------------------------------------------------------------------------------ (a) twin against scalar
@pytest.mark.parametrize("name", ti.SCALAR)
def test_twin_equals_the_scalar_loop(name):
    c = ti.case(name)
    states, cloud = ti.twin(name)
    nx, ny, nz = c.dims
    t, w = np.ones((nz, ny, nx), F32), np.zeros((nz, ny, nx), F32)
    hits, seen = set(), set()                # the pixels that voxels read, and their values
    for k, (depth, pose) in enumerate(c.frames):
        mine = set()
        ti.scalar_integrate(t, w, c, depth, pose, mine)
        ti.assert_same_state((t, w), states[k], (name, k))
        hits |= mine
        seen |= {int(depth[v, u]) for v, u in mine}
    xyz, edge = ti.scalar_extract(t, w, c.origin, c.voxel, c.min_weight)
    ti.assert_same_cloud((xyz, edge), cloud, name)
    assert (np.diff(cloud.edge) > 0).all() and cloud.xyz.flags.c_contiguous
    t, w = states[-1]
    H, W = c.frames[0][0].shape
    if name == "outside":
        assert (t == 1).all() and (w == 0).all() and cloud.xyz.shape == (0, 3) and cloud.edge.shape == (0,)
    if name == "behind":                     # layers k = 0 .. 2 have c_z <= 0
        assert (w[:3] == 0).all() and (w[3:] > 0).any() and (w[3:] == 0).any()
    if name == "centre-plane":
        assert np.argwhere(w > 0).tolist() == [[0, 3, 4]] and hits == {(int(c.camera.ppy + F32(0.5)), int(c.camera.ppx + F32(0.5)))}
    if name == "borders":                    # the [-0.5, W - 0.5) rule: the first and last row and column are reached
        vs, us = {v for v, _ in hits}, {u for _, u in hits}
        assert min(us) == 0 and max(us) == W - 1 and min(vs) == 0 and max(vs) == H - 1
        assert len(hits) < nx * ny           # and some voxels project beyond them
    if name == "trunc-edges":
        assert (w[:11] == 1).all() and (w[11:] == 0).all() and (t[11:] == 1).all()
        assert (t[10] == -1).all() and (t[:2] == 1).all() and (t[6] == 0).all() and (np.abs(t[3:10]) < 1).all()
    if name == "saturate":
        assert [float(s[1].max()) for s in states] == [1, 2, 2, 2, 2] and set(np.unique(w)) == {0.0, 2.0}
        assert cloud.xyz.shape[0] > 0
    if name == "13x11x9":                    # zero pixels and pixels beyond z_hi were met, and both frames wrote
        assert {0, 2600} <= seen and set(np.unique(w)) >= {0.0, 1.0, 2.0}


@pytest.mark.parametrize("name", ti.PLANTED_SCALAR)
def test_extraction_of_planted_states_equals_the_scalar_loop(name):
    t, w, origin, voxel, min_weight, _ = ti.planted(name)
    want = ti.scalar_extract(t, w, origin, voxel, min_weight)
    ti.assert_same_cloud(want, ti.planted_twin(name), name)


def test_designed_crossings():
    t, w, origin, voxel, min_weight, _ = ti.planted("designed")
    cloud = ti.planted_twin("designed")
    nz, ny, nx = t.shape

    def edge(ijk, a):
        i, j, k = ijk
        return 3 * ((k * ny + j) * nx + i) + a

    def point(ijk, a):
        return cloud.xyz[cloud.edge.tolist().index(edge(ijk, a))]

    have = set(cloud.edge.tolist())
    assert {edge(ti.P_ALL3, a) for a in range(3)} <= have                       # one voxel, three points
    assert {edge((3, 2, 1), 0), edge((4, 1, 1), 1)} <= have                     # towards the last voxel of every axis ...
    assert not {edge(ti.P_LAST, a) for a in range(3)} & have                    # ... which has no neighbour of its own
    centre = [F32(o) + (F32(i) + F32(0.5)) * F32(voxel) for o, i in zip(origin, ti.P_F0)]
    assert point(ti.P_F0, 0).tolist() == centre                                 # f = 0: the centre itself
    p = point(ti.P_F1, 0)
    assert p[0] == (F32(origin[0]) + F32(0.5) * F32(voxel)) + F32(1) * F32(voxel)   # f = 1: one voxel further
    assert edge(ti.P_ZEROS, 0) not in have                                      # 0.0 against 0.0
    assert not {edge(ti.P_NEGZERO, a) for a in range(3)} & have                 # -0.0 is not negative
    assert not {edge(ti.P_LIGHT, a) for a in range(3)} & have and edge((2, 2, 0), 0) not in have and edge((3, 1, 0), 1) not in have
    assert edge((4, 1, 0), 1) in have                                           # exactly min_weight takes part
    assert ti.planted_twin("random-13x11x9").xyz.shape[0] > 300 and ti.planted_twin("random-1x1x1").xyz.shape == (0, 3)


# ------------------------------------------------------------------------------------------------ (b) geometry
def test_fused_sphere_lies_on_the_sphere():
    """A sphere of radius 0.08 at 0.35 m, rendered analytically into 72 x 96 frames from three poses and fused into 32^3
    voxels of 0.01.  The bound is twice the largest distance the twin was measured to give against the analytic sphere:
    0.229 of a voxel at min_weight=1 (414 points) and 0.115 at min_weight=2 (319 points)."""
    c = ti.case("sphere")
    vol = ti.volume(c)
    for depth, pose in c.frames:
        vol.integrate(depth, c.camera, pose, c.z_range)
    for min_weight, bound, points in ((1, 2 * 0.229, 414), (2, 2 * 0.115, 319)):
        cloud = vol.extract(min_weight)
        off = np.abs(np.linalg.norm(cloud.xyz.astype(np.float64) - ti.SPHERE_C, axis=1) - ti.SPHERE_R) / c.voxel
        print(f"min_weight={min_weight}: {cloud.xyz.shape[0]} points, at most {off.max():.3f} of a voxel off the sphere")
        assert off.max() <= bound
        assert abs(cloud.xyz.shape[0] - points) <= points // 10
        assert (np.diff(cloud.edge) > 0).all() and cloud.edge.dtype == np.int64 and cloud.xyz.dtype == F32


# ------------------------------------------------------------------------------------------------ (c) state and refusals
def test_reset_and_state():
    T = _T()
    c = ti.case("5x3x2")
    vol = ti.volume(c)
    assert vol.shape == (2, 3, 5) and vol.tsdf.dtype == F32 and (vol.tsdf == 1).all() and (vol.weight == 0).all()
    assert vol.trunc == F32(4) * F32(c.voxel) and vol.origin == tuple(F32(o) for o in c.origin) and vol.max_weight == 64
    assert vol.extract().xyz.shape == (0, 3)
    vol.integrate(*c.frames[0][:1], c.camera)
    assert (vol.weight > 0).any()
    vol.reset()
    assert (vol.tsdf == 1).all() and (vol.weight == 0).all()
    # pose=None is the identity, and a torch frame on the host is taken
    a, b = ti.volume(c), ti.volume(c)
    a.integrate(c.frames[0][0], c.camera)
    b.integrate(torch.from_numpy(np.array(c.frames[0][0])), c.camera, np.eye(4))
    ti.assert_same_state((a.tsdf, a.weight), (b.tsdf, b.weight))
    # the twelve floats: R^T row-major, then -(R^T t), rounded once
    P = ti.pose(10.0, -20.0, 30.0, (0.1, -0.2, 0.3))
    assert [F32(x) for x in T.world_to_camera(P)] == ti.scalar_w2c(P)


def test_refusals():
    T = _T()
    from randlanet.utils.depth import DepthCamera
    ok = dict(origin=(0, 0, 0), voxel=0.01, dims=(4, 4, 4), device="cpu")
    for key, values, match in (("voxel", (0.0, -1.0, float("nan"), float("inf"), None, "1"), "voxel="),
                               ("trunc", (0.0, -0.1, float("nan"), float("inf")), "trunc="),
                               ("dims", ((4, 4), (0, 4, 4), (4, 4, -1), (4, 2.5, 4), (2048, 1024, 1024), "abc", 4), "dims"),
                               ("max_weight", (0, 65536, 1.5, None, True), "max_weight="),
                               ("origin", ((0, 0), (0, 0, float("nan")), "abc"), "origin")):
        for value in values:
            with pytest.raises(ValueError, match=match):
                T.TsdfVolume(**{**ok, key: value})
    with pytest.raises(ValueError, match="trunc="):                   # 4 * voxel overflows
        T.TsdfVolume(**{**ok, "voxel": 1e38})
    assert T.TsdfVolume(**{**ok, "max_weight": 65535}).max_weight == 65535
    c = ti.case("5x3x2")
    vol = ti.volume(c)
    frame, cam = c.frames[0][0], c.camera
    before = (vol.tsdf.copy(), vol.weight.copy())
    for bad, match in ((frame.astype(np.int16), "dtype int16"), (frame[:, :40], r"expected \(36, 48\)"), (frame[0], r"expected \(H, W\)"),
                       ([[1]], "numpy array or a torch tensor")):
        with pytest.raises(ValueError, match=match):
            vol.integrate(bad, cam)
    for z_range in ((0.6, 0.05), (0.3, 0.3), (0.1,), "ab"):
        with pytest.raises(ValueError, match="z_range="):
            vol.integrate(frame, cam, z_range=z_range)
    with pytest.raises(ValueError, match="coeffs"):
        vol.integrate(frame, DepthCamera(48, 36, 50.0, 50.0, 24.0, 18.0, ti.SCALE, (0.1, 0.0, 0.0, 0.0, 0.0)))
    with pytest.raises(ValueError, match="camera="):
        vol.integrate(frame, None)
    with pytest.raises(ValueError, match="below 2\\^24"):
        vol.integrate(frame, DepthCamera(2 ** 24, 1, 50.0, 50.0, 24.0, 18.0, ti.SCALE))
    scaled = np.eye(4)
    scaled[:3, :3] *= 1.01
    for pose in (np.eye(3), scaled, np.full((4, 4), np.nan), "pose"):
        with pytest.raises(ValueError, match="pose"):
            vol.integrate(frame, cam, pose)
    for min_weight in (0, 65, 1.5, None):
        with pytest.raises(ValueError, match="min_weight="):
            vol.extract(min_weight)
    ti.assert_same_state((vol.tsdf, vol.weight), before)              # nothing was written on the way


# ------------------------------------------------------------------------------------------------ (d) the camera loop
@pytest.fixture(scope="module")
def cpu_model():
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    return Model(RandLANetSettings(n_classes=4, n_points=512, n_neighbors=8, layer_sizes=[8, 16, 32, 32]), use_gpu=False)


def test_depth_fusion_with_given_poses(cpu_model):
    T = _T()
    c = ti.case("sphere")
    fusion = T.DepthFusion(cpu_model, c.camera, ti.volume(c), z_range=c.z_range)
    assert fusion.transformations.shape == (0, 4, 4)
    status = []
    for depth, pose in c.frames:
        res = fusion.add(depth, pose)
        assert isinstance(res, T.FusedFrame) and res.integrated and res.fitness == 1.0 and res.inlier_rmse == 0.0
        assert res.transformation.dtype == np.float64 and np.array_equal(res.transformation, pose)
        status.append(res.status)
    assert status == ["reference", "given", "given"]
    assert np.array_equal(fusion.transformations, np.array([p for _, p in c.frames]))
    states, cloud = ti.twin("sphere")
    ti.assert_same_state((fusion.volume.tsdf, fusion.volume.weight), states[-1])
    ti.assert_same_cloud(fusion.surface(), cloud)
    np.random.seed(3)
    got = fusion.predict(batch_size=2, pad_small_scenes=True)       # (414 points: below the network's 512)
    np.random.seed(3)
    want = cpu_model.predict_scene(fusion.volume.extract(1).xyz, None, batch_size=2, pad_small_scenes=True)
    assert isinstance(got, T.FusedPrediction) and got.confidences.shape == (4, cloud.xyz.shape[0]) and got.confidences.dtype == F32
    assert np.array_equal(got.confidences.view(np.uint32), want.view(np.uint32))
    ti.assert_same_cloud((got.xyz, got.edge), cloud)
    with pytest.raises(ValueError, match="needs its pose"):
        fusion.add(c.frames[0][0])
    assert fusion.transformations.shape == (3, 4, 4)
    for name in ("return_counts", "return_outliers", "return_planes"):
        with pytest.raises(ValueError, match=f"{name} is not taken"):
            fusion.predict(**{name: True})
    with pytest.raises(ValueError, match="no pixel inside z_range"):
        fusion.add(np.zeros(ti.LARGE, np.uint16), np.eye(4))
    fusion.reset()
    assert fusion.transformations.shape == (0, 4, 4) and (fusion.volume.weight == 0).all() and (fusion.volume.tsdf == 1).all()
    with pytest.raises(ValueError, match="the surface is empty"):
        fusion.predict()
    # frame 0 without a pose is the identity
    assert np.array_equal(fusion.add(c.frames[0][0]).transformation, np.eye(4))


def test_depth_fusion_with_a_temporal_filter(cpu_model):
    """Tracking and integration both see the filtered frame, and reset() clears the filter."""
    T = _T()
    from randlanet.utils.depth import TemporalFilter
    c = ti.case("13x11x9")
    noisy = [c.frames[0][0], np.where(c.frames[0][0] > 0, c.frames[0][0] + 7, 0).astype(np.uint16)]
    fusion = T.DepthFusion(cpu_model, c.camera, ti.volume(c), temporal=TemporalFilter())
    twin_filter, vol = TemporalFilter(), ti.volume(c)
    for frame in noisy:
        fusion.add(frame, np.eye(4))
        vol.integrate(twin_filter.process(frame, device="cpu"), c.camera)
    ti.assert_same_state((fusion.volume.tsdf, fusion.volume.weight), (vol.tsdf, vol.weight))
    assert not np.array_equal(twin_filter.process(noisy[1], device="cpu"), noisy[1])        # (the filter did something)
    fusion.reset()
    assert fusion.temporal.state is None


def test_depth_fusion_tracks_frame_to_model(cpu_model):
    """Three frames of the sphere on a ground plane from planted poses a few degrees and up to 2 cm apart, each tracked from
    the previous pose.  The scene keeps one symmetry - turning about the plane's normal through the sphere's centre - so the
    planted motion is pitch, roll, height and depth, along which a pose is determined.  The bounds are twice what the twin was
    measured to give: 0.730 and 0.185 degrees, 4.1 and 1.4 mm for frames 1 and 2."""
    T = _T()
    from randlanet.utils.registration import IcpSettings
    c = ti.sphere_case(ground=True, poses=ti.TRACK_POSES)
    fusion = T.DepthFusion(cpu_model, c.camera, ti.volume(c), icp=IcpSettings(max_distance=0.02))
    for k, (depth, pose) in enumerate(c.frames):
        res = fusion.add(depth)
        dT = np.linalg.inv(pose) @ res.transformation
        angle = np.degrees(np.arccos(np.clip((np.trace(dT[:3, :3]) - 1) / 2, -1, 1)))
        shift = np.linalg.norm(res.transformation[:3, 3] - pose[:3, 3])
        print(f"frame {k}: {res.status}, fitness {res.fitness:.3f}, rmse {res.inlier_rmse:.4f}, {angle:.3f} degrees and {1e3 * shift:.1f} mm off")
        if k == 0:
            assert res.status == "reference" and np.array_equal(res.transformation, np.eye(4))
            continue
        assert res.status in ("converged", "iterations") and res.integrated
        assert angle <= 2 * 0.730 and shift <= 2 * 0.0041
        assert res.fitness > 0.85 and res.inlier_rmse < 0.01
        # it moved towards the planted pose from where it started
        start = fusion.transformations[k - 1]
        assert shift < np.linalg.norm(start[:3, 3] - pose[:3, 3])
    # a given pose is the init, and a surface too small for the ICP's normals is ICP's own refusal
    assert fusion.add(c.frames[2][0], c.frames[2][1]).status in ("converged", "iterations")
    tiny = ti.case("1x1x1")
    few = T.DepthFusion(cpu_model, tiny.camera, ti.volume(tiny), icp=IcpSettings(max_distance=0.02))
    few.add(tiny.frames[0][0])
    with pytest.raises(ValueError, match="target"):
        few.add(tiny.frames[0][0])


def test_depth_fusion_refusals(cpu_model):
    T = _T()
    from randlanet.utils.depth import DepthCamera
    c = ti.case("5x3x2")
    vol = ti.volume(c)
    for kw, match in ((dict(icp=0.02), "icp="), (dict(temporal=0.33), "temporal="), (dict(z_range=(0.6, 0.05)), "z_range="),
                      (dict(track_stride=0), "stride="), (dict(min_weight=0), "min_weight="), (dict(min_weight=65), "min_weight=")):
        with pytest.raises(ValueError, match=match):
            T.DepthFusion(cpu_model, c.camera, vol, **kw)
    with pytest.raises(ValueError, match="volume="):
        T.DepthFusion(cpu_model, c.camera, None)
    with pytest.raises(ValueError, match="model="):
        T.DepthFusion(None, c.camera, vol)
    with pytest.raises(ValueError, match="coeffs"):
        T.DepthFusion(cpu_model, DepthCamera(48, 36, 50.0, 50.0, 24.0, 18.0, ti.SCALE, (0.1, 0.0, 0.0, 0.0, 0.0)), vol)
    fusion = T.DepthFusion(cpu_model, c.camera, vol)
    with pytest.raises(ValueError, match=r"expected \(36, 48\)"):
        fusion.add(np.zeros((36, 47), np.uint16))
    with pytest.raises(ValueError, match="pose"):
        fusion.add(c.frames[0][0], np.eye(3))
    assert fusion.transformations.shape == (0, 4, 4) and (vol.weight == 0).all()


# ------------------------------------------------------------------------------------------------ (e) the library's refusals
def test_host_side_refusals_of_the_entries():
    """Every refusal is made on the host, before any launch: no GPU is needed to see it."""
    from randlanet import _hip
    L = _hip.lib()
    assert L.rl_tsdf_workspace_bytes(0) == 0 and L.rl_tsdf_workspace_bytes(-1) == 0 and L.rl_tsdf_workspace_bytes(2 ** 31) == 0
    assert L.rl_tsdf_workspace_bytes(1) == 256 and L.rl_tsdf_workspace_bytes(1024 * 64 + 1) == 512
    assert L.rl_tsdf_workspace_bytes(2 ** 31 - 1) == 4 * 2 ** 21
    origin = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    rt = (ctypes.c_float * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    nan = float("nan")
    p, q = 4096, 8192                                  # (stand-ins for device pointers: never dereferenced by a refusal)

    def integrate(**kw):
        a = dict(tsdf=p, weight=q, nx=4, ny=4, nz=4, origin=origin, voxel=0.01, trunc=0.04, max_weight=64, depth=p, W=48, H=36,
                 fx=50.0, fy=50.0, ppx=24.0, ppy=18.0, scale=0.00025, z_lo=0.05, z_hi=0.6, rt=rt)
        a.update(kw)
        return L.rl_tsdf_integrate(a["tsdf"], a["weight"], a["nx"], a["ny"], a["nz"], a["origin"], a["voxel"], a["trunc"],
                                   a["max_weight"], a["depth"], a["W"], a["H"], a["fx"], a["fy"], a["ppx"], a["ppy"], a["scale"],
                                   a["z_lo"], a["z_hi"], a["rt"], None)

    bad_rt = (ctypes.c_float * 12)(*([1.0] * 11 + [nan]))
    bad_origin = (ctypes.c_float * 3)(0.0, float("inf"), 0.0)
    for kw in (dict(tsdf=None), dict(weight=None), dict(depth=None), dict(origin=None), dict(rt=None), dict(tsdf=p + 2), dict(weight=q + 1),
               dict(depth=p + 1), dict(nx=0), dict(nz=-1), dict(nx=2048, ny=1024, nz=1024), dict(nx=65536, ny=65536, nz=1),
               dict(voxel=0.0), dict(voxel=nan), dict(trunc=0.0), dict(trunc=float("inf")), dict(max_weight=0), dict(max_weight=65536),
               dict(W=0), dict(H=0), dict(W=2 ** 24), dict(W=2 ** 23, H=2 ** 8), dict(fx=0.0), dict(fy=nan), dict(scale=-1.0), dict(ppx=nan),
               dict(z_lo=0.6, z_hi=0.6), dict(z_lo=nan), dict(rt=bad_rt), dict(origin=bad_origin)):
        assert integrate(**kw) == _hip.ERR_ARGS, kw
        assert L.rl_last_error().startswith(b"rl_tsdf_integrate: "), kw

    def count(**kw):
        a = dict(tsdf=p, weight=q, nx=4, ny=4, nz=4, origin=origin, voxel=0.01, min_weight=1, count=p, ws=q, ws_bytes=256)
        a.update(kw)
        return L.rl_tsdf_count(a["tsdf"], a["weight"], a["nx"], a["ny"], a["nz"], a["origin"], a["voxel"], a["min_weight"], a["count"],
                               a["ws"], a["ws_bytes"], None)

    for kw in (dict(tsdf=None), dict(weight=None), dict(origin=None), dict(count=None), dict(ws=None), dict(ws=q + 128), dict(ws_bytes=255),
               dict(nx=64, ny=64, nz=17, ws_bytes=256), dict(min_weight=0), dict(min_weight=65536), dict(ny=0), dict(voxel=-0.01),
               dict(tsdf=p + 1), dict(nx=2048, ny=1024, nz=1024, ws_bytes=2 ** 24)):
        assert count(**kw) == _hip.ERR_ARGS, kw
        assert L.rl_last_error().startswith(b"rl_tsdf_count: "), kw

    def points(**kw):
        a = dict(tsdf=p, weight=q, nx=4, ny=4, nz=4, origin=origin, voxel=0.01, min_weight=1, count=10, xyz=p, edge=q, capacity=10, ws=q,
                 ws_bytes=256)
        a.update(kw)
        return L.rl_tsdf_points(a["tsdf"], a["weight"], a["nx"], a["ny"], a["nz"], a["origin"], a["voxel"], a["min_weight"], a["count"],
                                a["xyz"], a["edge"], a["capacity"], a["ws"], a["ws_bytes"], None)

    for kw in (dict(tsdf=None), dict(xyz=None), dict(edge=None), dict(ws=None), dict(ws_bytes=0), dict(count=0), dict(count=-1),
               dict(count=193), dict(count=11), dict(capacity=9), dict(count=2 ** 32, capacity=2 ** 32), dict(xyz=p + 2), dict(edge=q + 4),
               dict(min_weight=0), dict(nz=0), dict(voxel=0.0)):
        assert points(**kw) == _hip.ERR_ARGS, kw
        assert L.rl_last_error().startswith(b"rl_tsdf_points: "), kw
