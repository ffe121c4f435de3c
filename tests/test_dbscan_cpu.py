"""DBSCAN's density rule (min_samples) in the numpy twin of the clustering (utils/cluster.py) against the O(M^2) definition of
tests/dbscan_inputs.py on every named case, the properties each case was built for, min_samples = 1 against the clustering as
it was, and the refusals."""
import numpy as np
import pytest

import cluster_inputs as ci
import dbscan_inputs as di

F32 = np.float32


@pytest.mark.parametrize("name", di.CASES)
def test_twin_equals_the_definition(name):
    res, support, core, border = di.brute(name)
    ci.assert_same(di.twin(name), res, name)


@pytest.mark.parametrize("name", ci.CASES)
def test_min_samples_1_is_the_clustering_as_it_was(name):
    from randlanet.utils.cluster import euclidean_clusters_host
    xyz, lab, r, kw = ci.case(name)
    got = euclidean_clusters_host(xyz, lab, radius=r, scores=ci.scores_of(name), min_samples=1, **kw)
    ci.assert_same(got, ci.twin(name), name)
    ci.assert_same(got, ci.brute(name), name)


def _inst(name):
    return di.twin(name).instance


def test_bridge():
    xyz, _, _ = di.case("bridge_ms4")
    one, two = di.twin("bridge_ms1"), di.twin("bridge_ms4")
    assert one.count.tolist() == [85] and (one.instance == 0).all()
    assert sorted(two.count.tolist()) == [41, 41]             # each blob with the end of the chain that touches it
    chain = np.flatnonzero((xyz[:, 1] == F32(0.1)) & (xyz[:, 2] == 0) & (xyz[:, 0] > 0.3) & (xyz[:, 0] < 1.3))
    chain = chain[np.argsort(xyz[chain, 0])]
    assert chain.shape == (5,)
    _, support, core, border = di.brute("bridge_ms4")
    assert support[chain].tolist() == [3, 3, 3, 3, 3] and border[chain].tolist() == [True, False, False, False, True]
    left = two.instance[np.flatnonzero(xyz[:, 0] < 0.2)]
    right = two.instance[np.flatnonzero(xyz[:, 0] > 1.3)]
    assert len(set(left)) == 1 and len(set(right)) == 1 and left[0] != right[0]
    assert two.instance[chain].tolist() == [left[0], -1, -1, -1, right[0]]


def test_border_rule():
    # a tie, bit for bit: the lower core index (B's point 0) wins although A's cells are scanned first
    xyz, _, kw = di.case("border_tie_ms4")
    r2 = F32(kw["radius"]) * F32(kw["radius"])
    d = xyz[8] - xyz[[0, 4]]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert d2.dtype == F32 and d2[0].tobytes() == d2[1].tobytes() and d2[0] <= r2
    assert _inst("border_tie_ms4").tolist() == [0] * 4 + [1] * 4 + [0]
    # the higher-indexed core strictly nearer: it wins
    assert _inst("border_nearest_ms4").tolist() == [0] * 4 + [1] * 4 + [1]
    # the only link of two components is a border point: they stay two
    res = di.twin("border_no_bridge_ms4")
    assert res.count.tolist() == [5, 4] and res.instance.tolist() == [0] * 4 + [1] * 4 + [0]
    for name in ("border_tie_ms4", "border_nearest_ms4", "border_no_bridge_ms4"):
        _, support, core, border = di.brute(name)
        # (the border point counts for the two core points it touches; itself it reaches those two only)
        assert support.tolist() == [5, 4, 4, 4] * 2 + [3] and core.tolist() == [True] * 8 + [False] and border[8]


def test_numbering_goes_by_core_points():
    res = di.twin("border_is_smallest_index_ms4")
    assert res.instance.tolist() == [1] + [0] * 4 + [1] * 4 and res.count.tolist() == [4, 5]
    assert di.brute("border_is_smallest_index_ms4")[3].tolist() == [True] + [False] * 8


def test_border_points_count_for_min_points():
    kept, dropped = di.twin("border_counts_for_min_points_6_ms4"), di.twin("border_counts_for_min_points_7_ms4")
    assert kept.instance.tolist() == [0] * 6 + [1] * 8 and kept.count.tolist() == [6, 8]
    assert dropped.instance.tolist() == [-1] * 6 + [0] * 8 and dropped.count.tolist() == [8]
    _, support, core, border = di.brute("border_counts_for_min_points_6_ms4")
    assert core[:6].tolist() == [True] * 4 + [False] * 2 and border[4:6].all()


def test_support_counts_its_own_label_only():
    _, support, _, _ = di.brute("other_labels_do_not_count_ms2")
    assert support[0] == 1
    assert _inst("other_labels_do_not_count_ms1")[0] == 0 and _inst("other_labels_do_not_count_ms2")[0] == -1
    assert (_inst("other_labels_do_not_count_ms2")[4:10] == -1).all()        # ignored and unlabelled


def test_nothing_and_little():
    res = di.twin("all_noise_ms51")
    assert (res.instance == -1).all() and res.instance.dtype == np.int32 and res.instance.shape == (50,)
    assert res.classes.shape == (0,) and res.classes.dtype == np.int64
    assert res.count.shape == (0,) and res.count.dtype == np.int32
    assert res.centroid.shape == res.lo.shape == res.hi.shape == (0, 3) and res.score.shape == (0,)
    assert res.centroid.dtype == res.lo.dtype == res.hi.dtype == res.score.dtype == F32
    assert _inst("single_ms1").tolist() == [0] and _inst("single_ms2").tolist() == [-1]
    assert _inst("duplicates_ms5").tolist() == [0] * 5 and _inst("duplicates_ms6").tolist() == [-1] * 5
    assert _inst("at_r_ms2").tolist() == [0, 0] and _inst("at_r_beyond_ms2").tolist() == [-1, -1]


@pytest.mark.parametrize("name, n", [("cells_27_ms27", 27), ("planar_ms27", 27), ("corner_ms8", 8)])
def test_all_27_cells_are_walked(name, n):
    from randlanet.utils import cluster as K
    xyz, lab, kw = di.case(name)
    _, support, core, border = di.brute(name)
    res = di.twin(name)
    groups = xyz.shape[0] // n
    # cells_27: the centre alone reaches all 27; planar: three points coincide at the centre; corner: all 8 reach each other
    n_core = {"cells_27_ms27": 1, "planar_ms27": 3, "corner_ms8": 16}[name]
    assert core.sum() == n_core and border.sum() == xyz.shape[0] - n_core
    assert (support[core] == n).all() and res.count.tolist() == [n] * groups and (res.instance >= 0).all()
    # the neighbours lie in that many different cells
    o, dims = K.cluster_geometry(xyz, K.cell_edge(F32(kw["radius"])))
    cells = np.floor((xyz - o) / K.cell_edge(F32(kw["radius"]))).astype(np.int64)
    want = {"cells_27_ms27": (27, [3, 3, 3]), "planar_ms27": (9, [3, 3, 1]), "corner_ms8": (16, None)}[name]
    assert len({tuple(c) for c in cells.tolist()}) == want[0] and (want[1] is None or dims.tolist() == want[1])
    if name == "corner_ms8":
        corners = {(0, 0, 0), tuple((dims - 1).tolist())}
        assert corners <= {tuple(c) for c in cells.tolist()} and (dims > 2).all()


@pytest.mark.parametrize("name", ["uniform_4097_ms2", "uniform_4097_ms5", "uniform_20000_ms2", "uniform_20000_ms5"])
def test_uniform_clouds_hold_every_kind_of_point(name):
    """At min_samples = 2 a point that is not core has no neighbour at all, so no border point can exist; at 5 all three do."""
    xyz, lab, kw = di.case(name)
    _, support, core, border = di.brute(name)
    part = (lab > 0)
    noise = part & ~core & ~border
    print(f"{name}: {int(core.sum())} core, {int(border.sum())} border, {int(noise.sum())} noise, "
          f"{di.twin(name).count.shape[0]} instances")
    assert core.sum() > 100 and noise.sum() > 100 and (~part).sum() > 100
    assert border.sum() == 0 if kw["min_samples"] == 2 else border.sum() > 100
    res = di.twin(name)
    assert np.array_equal(res.instance >= 0, core | border) and set(res.classes.tolist()) == {1, 2, 3}


@pytest.mark.parametrize("name", ["smooth_dense_ms4", "smooth_dense_curv_ms4"])
def test_smooth_rule_with_density(name):
    xyz, lab, kw = di.case(name)
    res = di.twin(name)
    _, support, core, border = di.brute(name)
    floor = xyz[:, 2] == 0
    assert res.count.shape == (2,)
    took_part = np.ones(72, bool) if "curvature" not in kw else ~(kw["curvature"] > F32(kw["max_curvature"]))
    assert np.array_equal(res.instance >= 0, took_part) and (~took_part).sum() == (0 if "curvature" not in kw else 12)
    assert len(set(res.instance[floor & took_part])) == 1 and len(set(res.instance[~floor & took_part])) == 1
    if "curvature" not in kw:
        # the floor point at the crease's end: support 4 with the wall's point, of which only 3 agree with its normal - core
        # all the same, because support counts the plain rule
        i = int(np.flatnonzero((xyz[:, 0] == 0) & (xyz[:, 1] == 0) & floor)[0])
        agree = np.abs(kw["normals"] @ kw["normals"][i]) > 0.5
        d = np.linalg.norm(xyz.astype(np.float64) - xyz[i].astype(np.float64), axis=1)
        assert support[i] == (d <= 0.25).sum() == 4 and (agree & (d <= 0.25)).sum() == 3 and core[i]
        assert border.sum() >= 1                              # (the plates' far corners reach two points only)


def test_refusals():
    from randlanet.utils.cluster import check_min_samples, euclidean_clusters_host
    xyz, lab = np.zeros((3, 3), F32), np.ones(3, np.int64)
    for bad in (0, -1, 1.5, "2", None, float("nan"), float("inf"), True):
        with pytest.raises(ValueError, match="min_samples"):
            euclidean_clusters_host(xyz, lab, radius=1.0, min_samples=bad)
    assert check_min_samples(np.int64(3)) == 3 and check_min_samples(2.0) == 2
    assert euclidean_clusters_host(xyz, lab, radius=1.0, min_samples=3).count.tolist() == [3]


def test_model_on_the_cpu_passes_min_samples_on():
    """predict_instances on a CPU-placed model: the twin with min_samples on the model's own votes; a bad one is refused
    before any vote."""
    import torch
    from randlanet.model import Model
    from randlanet.utils import cluster as K
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    model = Model(RandLANetSettings(n_classes=3, n_points=256, n_neighbors=4, layer_sizes=[8, 16]), use_gpu=False)
    xyz = np.random.RandomState(3).uniform(0, 2, (600, 3)).astype(F32)
    with pytest.raises(ValueError, match="min_samples"):
        model.predict_instances(xyz, radius=0.3, min_samples=0)
    kw = dict(radius=0.3, min_points=2, ignore_classes=(), seed=1)
    np.random.seed(5)
    got = model.predict_instances(xyz, min_samples=4, **kw)
    want = K.euclidean_clusters_host(xyz, got.label, radius=0.3, min_points=2, ignore_classes=(), scores=None, min_samples=4)
    assert np.array_equal(got.instance, want.instance) and np.array_equal(got.count, want.count)
    np.random.seed(5)
    plain = model.predict_instances(xyz, **kw)
    assert np.array_equal(plain.label, got.label) and not np.array_equal(plain.instance, got.instance)
