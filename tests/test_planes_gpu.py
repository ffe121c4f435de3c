"""RANSAC plane segmentation on the MI355X: csrc/planes.hip against the numpy twin (utils/planes.py) on every case of
tests/planes_inputs.py, bit for bit over every field; the entries' refusals, launches and workspace; and the `remove_planes=`
keyword of a GPU-placed Model's scene functions against the same steps done by hand."""
import numpy as np
import pytest
import torch

import planes_inputs as pi

pytestmark = pytest.mark.gpu
F32 = np.float32


def _dev():
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------ (a) kernels against twin
@pytest.mark.parametrize("name", pi.CASES)
def test_device_equals_the_twin(name):
    from randlanet import _hip
    from randlanet.utils.planes import fit_plane
    xyz, kw = pi.case(name)
    got = fit_plane(xyz, device=_dev(), **kw)
    if pi.twin(name).counts.max() >= 3:                 # the refinement ran: the split under the refined plane came last
        assert _hip.lib().rl_last_kernel() == b"pl_write"
    pi.assert_same(got, pi.twin(name), name)           # counts and hypotheses as bits, not only the final mask


def test_default_device_segmentation_and_remove():
    from randlanet.utils.planes import fit_plane, remove_planes, segment_planes
    xyz, kw = pi.case("table_2")
    pi.assert_same(fit_plane(xyz.astype(np.float64), **kw), pi.twin("table_2"))        # device=None: a GPU is available
    room, want = pi.room()[0], pi.room_twin()
    pi.assert_same_segmentation(segment_planes(room, device=_dev(), **pi.ROOM), want, "room")
    pi.assert_same_segmentation(segment_planes(room, **pi.ROOM), want, "room, default device")
    x, lab, seg = remove_planes(room, np.arange(7500), **pi.ROOM)
    pi.assert_same_segmentation(seg, want)
    assert np.array_equal(x, room[want.kept]) and np.array_equal(lab, want.kept)


# ------------------------------------------------------------------------------------------------ (b) the entries
def test_entries_refuse_bad_arguments_and_count_their_launches():
    from randlanet import _hip as H
    from randlanet.utils.planes import counts_host, hypotheses_host
    lib = H.lib()
    xyz, kw = pi.case("table_3")
    with torch.cuda.device(_dev()):
        M, T = xyz.shape[0], 65
        tri_h = np.random.default_rng(1).integers(0, M, (T, 3), dtype=np.int64)
        pts = torch.from_numpy(np.array(xyz)).to(_dev())
        tri = torch.from_numpy(tri_h).to(_dev())
        hyp = torch.zeros((T, 4), dtype=torch.float32, device=_dev())
        bad = torch.full((1,), 7, dtype=torch.int32, device=_dev())
        counts = torch.zeros(T, dtype=torch.int32, device=_dev())
        best = torch.zeros(2, dtype=torch.int32, device=_dev())
        inlier = torch.zeros(M, dtype=torch.uint8, device=_dev())
        slot = torch.zeros(M, dtype=torch.int32, device=_dev())
        kept = torch.zeros(M, dtype=torch.int64, device=_dev())
        n = torch.zeros(1, dtype=torch.int64, device=_dev())
        need = lib.rl_planes_workspace_bytes(M, T)
        ws = torch.zeros(need + 256, dtype=torch.uint8, device=_dev())
        torch.cuda.synchronize()
        before = lib.rl_launch_count()
        good_h = [pts.data_ptr(), M, tri.data_ptr(), T, None, 0.0, hyp.data_ptr(), bad.data_ptr(), None]
        for pos, value in ((0, None), (2, None), (6, None), (7, None), (1, 2), (1, 2 ** 31 - 1), (3, 0), (3, 65537),
                           (6, hyp.data_ptr() + 4)):
            args = list(good_h)
            args[pos] = value
            assert lib.rl_planes_hypotheses(*args) == H.ERR_ARGS, (pos, value)
        thr = 0.01
        good_c = [pts.data_ptr(), M, hyp.data_ptr(), T, thr, counts.data_ptr(), best.data_ptr(), ws.data_ptr(), need, None]
        for pos, value in ((0, None), (2, None), (5, None), (6, None), (7, None), (1, 2), (1, 2 ** 31 - 1), (3, 0), (3, 65537),
                           (4, 0.0), (4, -1.0), (4, float("nan")), (4, float("inf")), (7, ws.data_ptr() + 8), (8, need - 1),
                           (8, 0)):
            args = list(good_c)
            args[pos] = value
            assert lib.rl_planes_count(*args) == H.ERR_ARGS, (pos, value)
        good_s = [pts.data_ptr(), M, hyp.data_ptr(), best.data_ptr(), thr, inlier.data_ptr(), slot.data_ptr(), kept.data_ptr(),
                  n.data_ptr(), ws.data_ptr(), need, None]
        for pos, value in ((0, None), (2, None), (5, None), (6, None), (7, None), (8, None), (9, None), (1, 2),
                           (1, 2 ** 31 - 1), (4, 0.0), (4, float("nan")), (9, ws.data_ptr() + 8), (10, 0),
                           (10, lib.rl_planes_workspace_bytes(M, 1) - 1)):
            args = list(good_s)
            args[pos] = value
            assert lib.rl_planes_split(*args) == H.ERR_ARGS, (pos, value)
        assert lib.rl_launch_count() == before
        assert lib.rl_planes_hypotheses(*good_h) == 0 and lib.rl_launch_count() == before + 1
        assert lib.rl_last_kernel() == b"pl_hyp"
        assert lib.rl_planes_count(*good_c) == 0 and lib.rl_launch_count() == before + 4
        assert lib.rl_last_kernel() == b"pl_best"
        assert lib.rl_planes_split(*good_s) == 0 and lib.rl_launch_count() == before + 7
        assert lib.rl_last_kernel() == b"pl_write"
        torch.cuda.synchronize()
        # what the three entries wrote, against the twin's pieces on the same triples
        want_h = hypotheses_host(xyz, tri_h)
        want_c = counts_host(xyz, want_h, F32(thr))
        assert pi.same_floats(hyp.cpu().numpy(), want_h, F32) and np.array_equal(counts.cpu().numpy(), want_c)
        b = int(np.argmax(want_c))
        assert best.tolist() == [b, int(want_c[b])] and bad.item() == 0
        on = pi._inliers(xyz, want_h[b], F32(thr), False)
        assert np.array_equal(inlier.cpu().numpy().astype(bool), on) and n.item() == (~on).sum()
        assert np.array_equal(kept[:n.item()].cpu().numpy(), np.flatnonzero(~on))
        assert np.array_equal(slot.cpu().numpy(), np.where(on, -1, np.cumsum(~on) - 1))
        # a plane of its own instead of a row of the hypotheses; the axis rule from host memory
        one = torch.from_numpy(want_h[b].copy()).to(_dev())
        args = list(good_s)
        args[2], args[3] = one.data_ptr(), None
        inlier.zero_()
        assert lib.rl_planes_split(*args) == 0
        assert np.array_equal(inlier.cpu().numpy().astype(bool), on)
        import ctypes
        axis = (ctypes.c_float * 3)(0.0, 0.0, 1.0)
        args = list(good_h)
        args[4], args[5] = axis, float(F32(np.cos(np.radians(10.0))))
        assert lib.rl_planes_hypotheses(*args) == 0
        assert pi.same_floats(hyp.cpu().numpy(), hypotheses_host(xyz, tri_h, np.array([0, 0, 1], F32),
                                                                 F32(np.cos(np.radians(10.0)))), F32)
        # an index outside the cloud reads nothing: the hypothesis is invalid and the flag is set
        tri_bad = tri_h.copy()
        tri_bad[3, 1], tri_bad[9, 0] = M, -1
        tri.copy_(torch.from_numpy(tri_bad))
        assert lib.rl_planes_hypotheses(*good_h) == 0
        got = hyp.cpu().numpy()
        assert bad.item() == 1 and np.isnan(got[[3, 9]]).all()
        keep = np.ones(T, bool)
        keep[[3, 9]] = False
        assert pi.same_floats(got[keep], want_h[keep], F32)
    from randlanet import _ops as ops
    with torch.cuda.device(_dev()), pytest.raises(ValueError, match="triples hold an index outside"):
        ops.fit_plane(pts, tri_bad, thr)


def test_fit_plane_adds_the_stated_launches():
    """_ops.fit_plane: 1 + 3 + 3 launches of planes.hip, and 3 more for the split under the refined plane; the rest belongs
    to instance_boxes and torch."""
    from randlanet import _hip as H
    from randlanet import _ops as ops
    lib = H.lib()
    xyz, kw = pi.case("lattice")
    with torch.cuda.device(_dev()):
        pts = torch.from_numpy(np.array(xyz)).to(_dev())
        ids = torch.zeros(xyz.shape[0], dtype=torch.int32, device=_dev())
        before = lib.rl_launch_count()
        ops.instance_boxes(pts, ids, 1, return_moments=True)
        boxes = lib.rl_launch_count() - before
        before = lib.rl_launch_count()
        ops.fit_plane(pts, kw["triples"].astype(np.int64), 0.25)
        assert lib.rl_launch_count() - before == 10 + boxes


def test_workspace_bytes():
    from randlanet import _hip
    lib = _hip.lib()
    for M, T in ((-1, 8), (0, 8), (2, 8), (2 ** 31 - 1, 8), (2 ** 40, 8), (100, 0), (100, -1), (100, 65537)):
        assert lib.rl_planes_workspace_bytes(M, T) == 0, (M, T)
    for T in (1, 64, 65, 256, 1024, 65536):
        last = 0
        for M in (3, 63, 64, 255, 256, 257, 1023, 1024, 1025, 70000, 501221, 10 ** 7, 2 ** 31 - 2):
            n = lib.rl_planes_workspace_bytes(M, T)
            cap = max(8, min(1024, 2 ** 20 // T))                       # chunks of the table: at most cap, 256 points or more
            chunk = max(256, -(-(-(-M // cap)) // 64) * 64)
            chunks = -(-M // chunk)
            assert chunks <= cap and n % 256 == 0 and n >= last, (M, T)
            assert 4 * chunks * T + 4 * -(-M // 1024) <= n <= 4 * chunks * T + 4 * -(-M // 1024) + 512, (M, T)
            assert n <= 4 * max(2 ** 20, 8 * T) + 4 * -(-M // 1024) + 512, (M, T)
            last = n
    assert lib.rl_planes_workspace_bytes(10 ** 7, 1024) <= 5 * 2 ** 20                 # a scan at T = 1024: a few MB
    for M in (3, 1025, 70000):
        assert lib.rl_planes_workspace_bytes(M, 1) <= lib.rl_planes_workspace_bytes(M, 64) <= lib.rl_planes_workspace_bytes(M, 65536)


# ------------------------------------------------------------------------------------------------ (c) Model
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
    """A floor of 2500 points, 3500 points in a slab above it and 40 floating over both."""
    rs = np.random.RandomState(21)
    floor = np.concatenate([rs.uniform((0, 0), (5, 5), (2500, 2)), rs.normal(0, 0.004, (2500, 1))], axis=1)
    xyz = np.concatenate([floor, rs.uniform((0, 0, 0.1), (5, 5, 2.5), (3500, 3)), rs.uniform((0, 0, 4), (5, 5, 8), (40, 3))])
    return np.ascontiguousarray(xyz[rs.permutation(6040)], dtype=F32)


def _removal(**kw):
    from randlanet.utils.planes import PlaneRemoval
    return PlaneRemoval(**dict(dict(threshold=0.015, iterations=128, seed=3), **kw))


SEG = dict(threshold=0.015, iterations=128, seed=3)


@pytest.fixture(scope="module")
def peeled(scan):
    from randlanet.utils.planes import segment_planes_host
    seg = segment_planes_host(scan, **SEG)
    assert seg.planes.shape[0] == 1 and 2400 <= seg.counts[0] <= 2700 and abs(seg.planes[0, 2]) > 0.999
    return seg


KW = dict(votes=1, batch_size=4, seed=2)


def test_predict_scene_removes_what_the_caller_would(gpu_model, scan, peeled):
    np.random.seed(5)
    got, count, (planes, plane_id) = gpu_model.predict_scene(scan, remove_planes=_removal(), return_counts=True,
                                                             return_planes=True, **KW)
    np.random.seed(5)
    p, c = gpu_model.predict_scene(scan[peeled.kept], return_counts=True, **KW)
    want, wcount = np.zeros((3, 6040), F32), np.zeros(6040, c.dtype)
    want[:, peeled.kept], wcount[peeled.kept] = p, c
    assert pi.same_floats(planes, peeled.planes, F32) and np.array_equal(plane_id, peeled.plane_id)    # the twin's, on the device
    assert plane_id.dtype == np.int32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(count, wcount)
    with pytest.raises(ValueError, match="threshold"):
        gpu_model.predict_scene(scan, remove_planes=_removal(threshold=-1.0), **KW)
    with pytest.raises(ValueError, match="the scene has 2 points, fewer than the 3"):
        gpu_model.predict_scene(scan[:2], remove_planes=_removal(), pad_small_scenes=True, **KW)


def test_predict_scene_with_grid_outliers_and_normals(scan):
    from randlanet.utils.grid import grid_subsample
    from randlanet.utils.normals import normal_features
    from randlanet.utils.outliers import statistical_outliers
    from randlanet.utils.planes import segment_planes
    model = _model(n_features=4)
    sub = grid_subsample(scan, cell=0.12, device=_dev())
    out = statistical_outliers(sub.xyz, 8, 2.0, device=_dev())
    left = np.ascontiguousarray(sub.xyz[out.kept])
    seg = segment_planes(left, device=_dev(), **SEG)
    rest = np.ascontiguousarray(left[seg.kept])
    assert seg.planes.shape[0] == 1 and (~out.keep).any() and 2048 < rest.shape[0] < left.shape[0] < sub.xyz.shape[0] < 6040
    np.random.seed(5)
    got, removed, (planes, plane_id) = model.predict_scene(scan, grid=0.12, outliers=(8, 2.0), remove_planes=_removal(),
                                                           normals=8, return_outliers=True, return_planes=True, **KW)
    np.random.seed(5)
    p = model.predict_scene(rest, normal_features(rest, 8), **KW)              # normals of what is left only
    per_cell = np.zeros((3, sub.xyz.shape[0]), F32)
    per_cell[:, out.kept[seg.kept]] = p
    cell_plane = np.full(sub.xyz.shape[0], -1, np.int32)
    cell_plane[out.kept] = seg.plane_id
    assert np.array_equal(removed, ~out.keep[sub.inverse]) and removed.any()
    assert np.array_equal(plane_id, cell_plane[sub.inverse]) and pi.same_floats(planes, seg.planes, F32)
    assert np.array_equal(got.view(np.uint32), per_cell[:, sub.inverse].view(np.uint32))


def test_instances_and_keypoints_never_return_a_plane_point(gpu_model, scan, peeled):
    on = peeled.plane_id >= 0
    kw = dict(radius=0.3, min_points=3, ignore_classes=(), **KW)
    np.random.seed(5)
    res, (planes, plane_id) = gpu_model.predict_instances(scan, remove_planes=_removal(), oriented_boxes=True,
                                                          return_planes=True, **kw)
    np.random.seed(5)
    ref = gpu_model.predict_instances(scan[peeled.kept], oriented_boxes=True, **kw)
    assert np.array_equal(plane_id, peeled.plane_id) and res.instance.shape == (6040,) and res.count.shape[0] >= 1
    assert (res.instance[on] == -1).all() and (res.label[on] == -1).all() and (res.label[~on] >= 0).all()
    assert np.array_equal(res.instance[peeled.kept], ref.instance) and np.array_equal(res.label[peeled.kept], ref.label)
    assert all(np.array_equal(a, b) for a, b in zip(res[2:], ref[2:]))
    kw = dict(radius=0.5, min_score=0.0, ignore_classes=(), **KW)
    np.random.seed(5)
    kp = gpu_model.predict_keypoints(scan, remove_planes=_removal(), **kw)
    np.random.seed(5)
    kref = gpu_model.predict_keypoints(scan[peeled.kept], **kw)
    assert kp.index.shape[0] >= 1 and not on[kp.index].any()
    assert np.array_equal(kp.index, peeled.kept[kref.index])
    assert all(np.array_equal(a, b) for a, b in zip(kp[1:], kref[1:]))
    # a device tensor stays where it is and gives the same result
    np.random.seed(5)
    kd = gpu_model.predict_keypoints(torch.from_numpy(scan).to(gpu_model.device), remove_planes=_removal(), **kw)
    assert all(np.array_equal(a, b) for a, b in zip(kd, kp))
    np.random.seed(5)
    a = gpu_model.predict_scene(torch.from_numpy(scan).to(gpu_model.device), remove_planes=_removal(), **KW)
    np.random.seed(5)
    b = gpu_model.predict_scene(scan, remove_planes=_removal(), **KW)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_cpu_placed_model_removes_the_same_points(gpu_model, scan, peeled):
    from randlanet._scene_path import VoteOptions
    cpu_model = _model(use_gpu=False)
    _, checked = VoteOptions(remove_planes=_removal()).checked
    a, ia, (pa, ida) = gpu_model._scene_path.remove_planes(scan, None, checked, 3, False, "the scene")
    b, ib, (pb, idb) = cpu_model._scene_path.remove_planes(scan, None, checked, 3, False, "the scene")
    assert torch.is_tensor(a) and a.is_cuda and isinstance(b, np.ndarray) and b.shape == (peeled.kept.shape[0], 3)
    assert np.array_equal(a.cpu().numpy().view(np.uint32), b.view(np.uint32))
    assert np.array_equal(ia, ib) and np.array_equal(ib, peeled.slot) and np.array_equal(ida, idb)
    assert pi.same_floats(pa, pb, F32) and pi.same_floats(pb, peeled.planes, F32)
