"""RANSAC plane segmentation without a GPU: the numpy twin (utils/planes.py) against the independent yardstick of
tests/planes_inputs.py, the properties every case is there for (so a case cannot quietly stop testing anything), the
refusals, remove_planes, the triples' own generator, and the `remove_planes=` keyword of a CPU-placed Model."""
import numpy as np
import pytest
import torch

import planes_inputs as pi

F32 = np.float32


# ------------------------------------------------------------------------------------------------ 1. twin against yardstick
@pytest.mark.parametrize("name", pi.CASES)
def test_twin_equals_the_yardstick(name):
    from randlanet.utils.planes import refined_plane
    xyz, kw = pi.case(name)
    got, want = pi.twin(name), pi.yardstick(name)
    assert pi.same_floats(got.hypotheses, want["hypotheses"], F32), name
    assert got.counts.dtype == np.int32 and np.array_equal(got.counts, want["counts"]), name
    assert got.best == want["best"], name
    if want["best"] < 0:
        return
    thr, scalar = F32(kw["threshold"]), name in pi.SCALAR
    if got.counts[got.best] >= 3:
        # the refinement: the moments by the yardstick's own sums give the twin's plane through the shared float64 step;
        # numpy's eigh agrees with the contract's Jacobi sweeps to rounding (an exactly flat set leaves eigh's sign open)
        assert pi.same_floats(got.centroid, want["mean"], np.float64), name
        assert pi.same_floats(refined_plane(want["mean"], want["cov"]), got.plane, F32), name
        assert abs(abs(np.dot(got.plane[:3].astype(np.float64), want["normal"])) - 1.0) < 1e-6, name
        big = int(np.argmax(np.abs(got.plane[:3])))
        assert got.plane[big] > 0 and abs(np.linalg.norm(got.plane[:3].astype(np.float64)) - 1.0) < 1e-6
    else:
        assert pi.same_floats(got.plane, want["hypotheses"][want["best"]], F32) and np.isnan(got.centroid).all()
    final = pi._inliers(xyz, got.plane, thr, scalar)
    assert np.array_equal(got.inlier, final) and got.count == final.sum(), name
    assert np.array_equal(got.kept, np.flatnonzero(~final)) and got.kept.dtype == np.int64
    assert np.array_equal(got.slot, np.where(final, -1, np.cumsum(~final) - 1)) and got.slot.dtype == np.int32


# ------------------------------------------------------------------------------------------------ 2. what the cases are for
@pytest.mark.parametrize("seed", (1, 2, 3))
def test_table_is_found(seed):
    flag = pi.table(seed)[1]
    fit = pi.twin(f"table_{seed}")
    assert (~np.isnan(fit.hypotheses[:, 0])).sum() >= 250
    assert fit.inlier[flag].sum() >= 980 and fit.inlier[~flag].sum() <= 25
    assert np.abs(fit.plane[:3] - pi.NORMAL).max() < 1e-3 and abs(fit.plane[3] + pi.OFFSET) < 1e-3
    assert fit.count >= 3 and fit.counts[fit.best] == fit.counts.max() and (fit.counts[:fit.best] < fit.counts.max()).all()


def test_edge_shell_tells_fused_from_unfused():
    xyz, kw = pi.case("edge_shell")
    fit = pi.twin("edge_shell")
    assert np.array_equal(kw["triples"][0], [0, 1, 2]) and not np.isnan(fit.hypotheses[0]).any()
    h = fit.hypotheses[0].astype(np.float64)
    s = np.abs(xyz[700:].astype(np.float64) @ h[:3] + h[3])
    assert (np.abs(s - 0.01) < 6e-6).all()                      # the shell lies on the edge of hypothesis 0
    fused = pi.fused_counts("edge_shell")
    assert fused[0] != fit.counts[0] and 1000 < fit.counts[0] < 2600, (fused[0], fit.counts[0])


def test_lattice_distances_are_exact_and_the_edge_is_in():
    xyz, _ = pi.case("lattice")
    fit = pi.twin("lattice")
    assert np.array_equal(fit.hypotheses, np.tile(np.array([[0, 0, 1, 0]], F32), (4, 1)))
    assert (fit.counts == 192).all() and fit.best == 0 and fit.count == 192
    assert np.array_equal(fit.inlier, np.abs(xyz[:, 2]) <= 0.25)
    assert np.array_equal(np.abs(fit.plane), np.array([0, 0, 1, 0], F32))


def test_ties_go_to_the_lower_index():
    fit = pi.twin("ties")
    assert fit.counts.tolist() == [80, 192, 192, 192] and fit.best == 1
    assert np.array_equal(fit.hypotheses[1], fit.hypotheses[2]) and np.array_equal(fit.hypotheses[1], fit.hypotheses[3])


def test_degenerate_triples_and_clouds():
    fit = pi.twin("degenerate")
    assert np.isnan(fit.hypotheses[[0, 1, 2, 4]]).all() and not np.isnan(fit.hypotheses[3]).any()
    assert fit.counts[[0, 1, 2, 4]].tolist() == [0, 0, 0, 0] and fit.best == 3 and fit.counts[3] >= 3
    one = pi.twin("one_point")
    assert one.best == -1 and one.count == 0 and np.isnan(one.plane).all() and np.isnan(one.hypotheses).all()
    assert not one.inlier.any() and np.array_equal(one.kept, np.arange(50)) and np.array_equal(one.slot, np.arange(50))
    small = pi.twin("smallest")
    assert small.best == 0 and small.count == 3 and small.inlier.all() and small.kept.shape == (0,)
    assert pi.twin("t_65").counts.shape == (65,) and pi.twin("t_65").count >= 980


def test_axis_rule():
    free, tight, wide = pi.twin("table_1"), pi.twin("axis_10"), pi.twin("axis_30")
    valid = ~np.isnan(tight.hypotheses[:, 0])
    assert 0 < valid.sum() < 64 and (np.abs(tight.hypotheses[valid, 2]) >= F32(np.cos(np.radians(10.0)))).all()
    near = np.abs(free.hypotheses[:, :3].astype(np.float64) @ pi.NORMAL) > np.cos(np.radians(5.0))
    assert near.sum() >= 10 and np.isnan(tight.hypotheses[near]).all()         # every one near the true plane is invalid
    assert tight.count < 200
    assert wide.best == free.best and wide.count == free.count and np.array_equal(wide.plane, free.plane)
    assert np.array_equal(wide.inlier, free.inlier) and np.isnan(wide.hypotheses[:, 0]).sum() > 0
    assert not np.isnan(wide.hypotheses[near]).any()


def test_room_peels_three_planes():
    xyz, surface = pi.room()
    seg = pi.room_twin()
    assert seg.planes.shape == (3, 4) and seg.planes.dtype == F32 and seg.counts.dtype == np.int64
    assert sorted(int(np.bincount(surface[seg.plane_id == p]).argmax()) for p in range(3)) == [0, 1, 2]
    for p in range(3):
        on = surface[seg.plane_id == p]
        assert on.shape[0] == seg.counts[p] >= 500 and np.bincount(on).max() >= 0.95 * on.shape[0]
    assert seg.plane_id.dtype == np.int32 and np.array_equal(seg.kept, np.flatnonzero(seg.plane_id < 0))
    assert np.array_equal(seg.slot[seg.kept], np.arange(seg.kept.shape[0])) and (seg.slot[seg.plane_id >= 0] == -1).all()
    # the fourth round found something, below min_points: with min_points low it is a plane
    from randlanet.utils.planes import segment_planes_host
    more = segment_planes_host(xyz, **dict(pi.ROOM, min_points=3))
    assert more.planes.shape[0] == 4 and more.counts[3] < 500 and np.array_equal(more.planes[:3], seg.planes)
    one = segment_planes_host(xyz, **dict(pi.ROOM, max_planes=1))
    assert one.planes.shape[0] == 1 and np.array_equal(one.planes[0], seg.planes[0])


def test_many_chunks_finds_its_plane():
    fit = pi.twin("many_chunks")
    assert fit.count > 19000 and abs(fit.plane[2]) > 0.999 and abs(fit.plane[3] + 4.0) < 0.02


# ------------------------------------------------------------------------------------------------ 3. refusals, columns, rng
def test_refusals():
    from randlanet.utils.planes import fit_plane, fit_plane_host, remove_planes, segment_planes_host
    xyz = pi.case("table_1")[0]
    for fn in (fit_plane_host, lambda *a, **kw: fit_plane(*a, device="cpu", **kw)):
        for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60, 1e60, "x", None, True):
            with pytest.raises(ValueError, match="threshold"):
                fn(xyz, bad)
        for bad in (0, -1, 65537, 2.5, "8", None, True):
            with pytest.raises(ValueError, match="iterations"):
                fn(xyz, 0.01, bad)
        for bad in (xyz[:2], xyz[:, :2], xyz.reshape(-1), np.zeros((0, 3), F32)):
            with pytest.raises(ValueError, match="xyz"):
                fn(bad, 0.01)
        far = np.array(xyz)
        far[7, 1] = np.inf
        with pytest.raises(ValueError, match="xyz has non-finite coordinates, first at point 7"):
            fn(far, 0.01)
        for bad in (np.zeros((4, 2), np.int64), np.zeros((4, 3), F32), np.array([[0, 1, 1500]]), np.array([[-1, 0, 1]])):
            with pytest.raises(ValueError, match="triples"):
                fn(xyz, 0.01, triples=bad)
        for kw in (dict(axis=(0, 0, 1)), dict(max_angle=10), dict(axis=(0, 0, 0), max_angle=10),
                   dict(axis=(0, 0, np.nan), max_angle=10), dict(axis=(0, 1), max_angle=10)):
            with pytest.raises(ValueError, match="axis"):
                fn(xyz, 0.01, **kw)
        for bad in (0, -5, 90.5, float("nan"), "x"):
            with pytest.raises(ValueError, match="max_angle"):
                fn(xyz, 0.01, axis=(0, 0, 1), max_angle=bad)
    for bad in (0, 65, 1.5):
        with pytest.raises(ValueError, match="max_planes"):
            segment_planes_host(xyz, 0.01, max_planes=bad)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="min_points"):
            segment_planes_host(xyz, 0.01, min_points=bad)
    with pytest.raises(ValueError, match="column 0 has shape"):
        remove_planes(xyz, np.zeros(7), threshold=0.01, device="cpu")
    # an axis of any length is normalised; 90 degrees allows every plane
    a = fit_plane_host(xyz, 0.01, 32, axis=(0, 0, 250.0), max_angle=90)
    b = fit_plane_host(xyz, 0.01, 32)
    pi.assert_same(a, b)


def test_remove_carries_columns():
    from randlanet.utils.planes import remove_planes, segment_planes_host
    xyz = pi.room()[0].astype(np.float64)
    feat, lab = np.arange(7500 * 2, dtype=F32).reshape(7500, 2), np.arange(7500)
    want = pi.room_twin()
    x, f, l, seg = remove_planes(xyz, feat, lab, device="cpu", **pi.ROOM)
    pi.assert_same_segmentation(seg, want)
    assert x.dtype == np.float64 and np.array_equal(x, xyz[want.kept])
    assert f.dtype == F32 and np.array_equal(f, feat[want.kept]) and np.array_equal(l, want.kept)
    pi.assert_same_segmentation(segment_planes_host(xyz, **pi.ROOM), want)


def test_the_triples_come_from_their_own_generator():
    from randlanet.utils.planes import draw_triples, fit_plane_host, segment_planes_host
    xyz, kw = pi.case("table_2")
    np.random.seed(123)
    before = np.random.get_state()
    fit = fit_plane_host(xyz, **kw)
    segment_planes_host(xyz, 0.01, 2, 100, 64, seed=3)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    tri = draw_triples(np.random.default_rng(kw["seed"]), xyz.shape[0], kw["iterations"])
    assert tri.dtype == np.int64 and tri.shape == (256, 3)
    pi.assert_same(fit_plane_host(xyz, kw["threshold"], triples=tri), fit)
    # the peeling continues ONE generator: round two's triples are its next draw, over the points that are left
    rng = np.random.default_rng(3)
    first = fit_plane_host(xyz, 0.01, triples=draw_triples(rng, 1500, 64))
    rest = np.ascontiguousarray(xyz[first.kept])
    second = fit_plane_host(rest, 0.01, triples=draw_triples(rng, rest.shape[0], 64))
    seg = segment_planes_host(xyz, 0.01, 2, 3, 64, seed=3)
    assert np.array_equal(seg.planes, np.stack((first.plane, second.plane)))
    assert seg.counts.tolist() == [first.count, second.count]


# ------------------------------------------------------------------------------------------------ 4. CPU-placed model
@pytest.fixture(scope="module")
def cpu_model():
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    return Model(RandLANetSettings(n_classes=4, n_points=512, n_neighbors=8, layer_sizes=[8, 16, 32, 32]), use_gpu=False)


@pytest.fixture(scope="module")
def scan():
    """1000 points of the table and 800 above it."""
    xyz = np.ascontiguousarray(pi.table(4, 1000, 800)[0], dtype=F32)
    xyz.setflags(write=False)
    return xyz


KW = dict(votes=1, batch_size=2, seed=2)


def _removal(**kw):
    from randlanet.utils.planes import PlaneRemoval
    return PlaneRemoval(**dict(dict(threshold=0.01, iterations=128, seed=4), **kw))


def test_model_refusals_come_before_any_work(cpu_model, scan):
    fns = (cpu_model.predict_scene, lambda *a, **kw: cpu_model.predict_instances(*a, radius=0.1, **kw),
           lambda *a, **kw: cpu_model.predict_keypoints(*a, radius=0.1, **kw))
    for bad, match in ((_removal(threshold=0.0), "threshold"), (_removal(iterations=0), "iterations"),
                       (_removal(max_planes=65), "max_planes"), (_removal(min_points=0), "min_points"),
                       (_removal(axis=(0, 0, 1)), "axis"), ((0.01, 1), "must be a PlaneRemoval"), (0.01, "must be a PlaneRemoval")):
        for fn in fns:
            with pytest.raises(ValueError, match=match):
                fn(scan, remove_planes=bad, **KW)
    with pytest.raises(ValueError, match="the scene has 2 points, fewer than the 3"):
        cpu_model.predict_scene(scan[:2], remove_planes=_removal(), pad_small_scenes=True, **KW)


def test_predict_scene_equals_the_steps_by_hand(cpu_model, scan):
    from randlanet.utils.planes import segment_planes_host
    seg = segment_planes_host(scan, 0.01, iterations=128, seed=4)
    assert seg.planes.shape[0] == 1 and 950 < seg.counts[0] < 1100 and seg.kept.shape[0] >= 512
    np.random.seed(5)
    got, count, (planes, plane_id) = cpu_model.predict_scene(scan, remove_planes=_removal(), return_counts=True,
                                                             return_planes=True, **KW)
    np.random.seed(5)
    p, c = cpu_model.predict_scene(scan[seg.kept], return_counts=True, **KW)
    want, wcount = np.zeros((4, 1800), F32), np.zeros(1800, c.dtype)
    want[:, seg.kept], wcount[seg.kept] = p, c
    assert pi.same_floats(planes, seg.planes, F32) and plane_id.dtype == np.int32 and np.array_equal(plane_id, seg.plane_id)
    assert got.dtype == F32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert count.dtype == c.dtype and np.array_equal(count, wcount) and (count[plane_id < 0] >= 1).all()
    # without the keyword nothing changes, and return_planes reports no plane
    np.random.seed(5)
    a = cpu_model.predict_scene(scan, **KW)
    np.random.seed(5)
    b, (none, ids) = cpu_model.predict_scene(scan, return_planes=True, **KW)
    assert np.array_equal(a, b) and none.shape == (0, 4) and ids.shape == (1800,) and (ids == -1).all()
    # no plane of min_points points: nothing is removed
    np.random.seed(5)
    c1, (none, ids) = cpu_model.predict_scene(scan, remove_planes=_removal(min_points=1500), return_planes=True, **KW)
    assert none.shape == (0, 4) and (ids == -1).all() and np.array_equal(c1.view(np.uint32), a.view(np.uint32))


def test_predict_scene_with_grid_and_outliers_composes_the_slots(cpu_model, scan):
    from randlanet.utils.grid import grid_subsample_host
    from randlanet.utils.outliers import statistical_outliers_host
    from randlanet.utils.planes import segment_planes_host
    rs = np.random.RandomState(4)
    xyz = np.concatenate([scan, scan + F32(0.003) * rs.randn(1800, 3).astype(F32)])
    sub = grid_subsample_host(xyz, None, cell=0.04)
    out = statistical_outliers_host(sub.xyz, 8, 2.0)
    left = np.ascontiguousarray(sub.xyz[out.kept])
    seg = segment_planes_host(left, 0.01, iterations=128, seed=4)
    assert seg.planes.shape[0] == 1 and 0 < (~out.keep).sum() and seg.kept.shape[0] >= 512
    np.random.seed(5)
    got, removed, (planes, plane_id) = cpu_model.predict_scene(xyz, grid=0.04, outliers=(8, 2.0), remove_planes=_removal(),
                                                               return_outliers=True, return_planes=True, **KW)
    np.random.seed(5)
    p = cpu_model.predict_scene(left[seg.kept], **KW)
    per_cell = np.zeros((4, sub.xyz.shape[0]), F32)
    per_cell[:, out.kept[seg.kept]] = p
    cell_plane = np.full(sub.xyz.shape[0], -1, np.int32)
    cell_plane[out.kept] = seg.plane_id
    assert np.array_equal(removed, ~out.keep[sub.inverse])                     # the outlier mask holds the outliers only
    assert np.array_equal(plane_id, cell_plane[sub.inverse]) and pi.same_floats(planes, seg.planes, F32)
    assert np.array_equal(got.view(np.uint32), per_cell[:, sub.inverse].view(np.uint32))
    gone = removed | (plane_id >= 0)
    assert (got[:, gone] == 0).all() and np.allclose(got[:, ~gone].sum(0), 1.0, atol=1e-5)


def test_predict_instances_and_keypoints_leave_the_plane_out(cpu_model, scan):
    from randlanet.utils.planes import segment_planes_host
    seg = segment_planes_host(scan, 0.01, iterations=128, seed=4)
    on = seg.plane_id >= 0
    kw = dict(radius=0.15, min_points=3, ignore_classes=(), **KW)
    np.random.seed(5)
    got, (planes, plane_id) = cpu_model.predict_instances(scan, remove_planes=_removal(), return_planes=True, **kw)
    np.random.seed(5)
    ref = cpu_model.predict_instances(scan[seg.kept], **kw)
    assert np.array_equal(plane_id, seg.plane_id) and got.instance.shape == (1800,) and ref.count.shape[0] >= 1
    assert (got.instance[on] == -1).all() and (got.label[on] == -1).all()
    assert np.array_equal(np.flatnonzero(got.label == -1), np.flatnonzero(on))
    assert np.array_equal(got.instance[seg.kept], ref.instance) and np.array_equal(got.label[seg.kept], ref.label)
    assert all(np.array_equal(a, b) for a, b in zip(got[2:], ref[2:]))
    kw = dict(radius=0.3, min_score=0.0, ignore_classes=(), **KW)
    np.random.seed(5)
    kp = cpu_model.predict_keypoints(scan, remove_planes=_removal(), **kw)
    np.random.seed(5)
    kref = cpu_model.predict_keypoints(scan[seg.kept], **kw)
    assert kp.index.shape[0] >= 1 and not on[kp.index].any()
    assert np.array_equal(kp.index, seg.kept[kref.index])
    assert all(np.array_equal(a, b) for a, b in zip(kp[1:], kref[1:]))
