"""Euclidean clustering without a GPU: the numpy twin (utils/cluster.py) against the brute-force definition of
tests/cluster_inputs.py on every case, its refusals, numbering, min_points and ignore_classes, the empty result, the twin of
rl_scene_labels, Model.predict_instances on a CPU-placed model, and the C ABI of the new entries."""
import numpy as np
import pytest
import torch

import cluster_inputs as ci

F32 = np.float32


# ------------------------------------------------------------------------------------------- 1. twin == the definition
@pytest.mark.parametrize("name", ci.CASES)
def test_twin_equals_brute_force(name):
    res, want = ci.twin(name), ci.brute(name)
    ci.assert_same(res, want, name)
    M = ci.case(name)[0].shape[0]
    assert res.instance.shape == (M,) and res.instance.dtype == np.int32
    I = res.count.shape[0]
    assert res.instance.max(initial=-1) == I - 1
    assert np.array_equal(np.bincount(res.instance[res.instance >= 0], minlength=I), res.count)


def test_what_the_cases_are_there_for():
    """The expected shape of the answer, from the brute force: a case that no longer holds its edge shows here."""
    b = ci.brute
    assert b("single")["count"].tolist() == [1] and b("single")["classes"].tolist() == [3]
    assert b("pair_at_r")["count"].tolist() == [2]
    assert b("pair_beyond_r")["count"].tolist() == [1, 1]
    assert b("duplicates")["count"].tolist() == [3] * 7 + [2] * 33
    assert b("all_ignored")["count"].shape == (0,) and (b("all_ignored")["instance"] == -1).all()
    assert b("chain_3000")["count"].tolist() == [3000] and (b("chain_3000")["instance"] == 0).all()
    cut = b("chain_3000_cut")
    assert sorted(cut["count"].tolist()) == [1223, 1777] and cut["instance"][0] == 0
    assert b("touching_classes")["classes"].tolist() == [1, 2] and b("touching_classes")["count"].tolist() == [600, 600]
    assert b("blobs_just_apart")["count"].tolist() == [500, 500]
    assert b("one_cell_4096")["count"].tolist() == [4096]
    u = b("uniform_20000")["count"]
    assert u.shape == (1010,) and int((u >= 5).sum()) == 136 and int(u.max()) == 5361
    assert b("uniform_20000_min5")["count"].shape == (136,)
    assert 1 not in b("uniform_20000")["classes"]
    for name in ("lattice_r", "lattice_0999r", "lattice_r_far", "lattice_0999r_far"):
        c = b(name)["count"]
        assert c.shape[0] > 100 and c.max() > 1000, name
    w = b("wide_pairs")["count"]
    assert 0 < int((w == 2).sum()) < 1500 and int(w.max()) == 2


def test_the_cells_of_the_wide_case_nearly_reach_the_limit():
    from randlanet.utils import cluster as K
    xyz, _, r, _ = ci.case("wide_pairs")
    _, dims = K.cluster_geometry(xyz, K.cell_edge(F32(r)))
    assert 50000 < dims[0] < K.MAX_CLUSTER_DIM and 50000 < dims[1] < K.MAX_CLUSTER_DIM
    xyz, _, r, _ = ci.case("lattice_r_far")
    assert xyz.min() > 7990 and np.ptp(xyz, axis=0).max() < 4


# ------------------------------------------------------------------------------------ 2. numbering, min_points, ignore
def test_numbering_follows_the_smallest_member():
    from randlanet.utils.cluster import euclidean_clusters_host
    # three far-apart pairs, the members of the pair listed first coming last
    xyz = np.array([[10, 0, 0], [0, 0, 0], [20, 0, 0], [20.1, 0, 0], [0.1, 0, 0], [10.1, 0, 0], [30, 0, 0]], F32)
    lab = np.array([2, 1, 3, 3, 1, 2, 1])
    res = euclidean_clusters_host(xyz, lab, radius=0.2)
    assert res.instance.tolist() == [0, 1, 2, 2, 1, 0, 3]
    assert res.classes.tolist() == [2, 1, 3, 1] and res.count.tolist() == [2, 2, 2, 1]
    assert np.array_equal(res.lo[0], [10, 0, 0]) and np.array_equal(res.hi[0], np.array([10.1, 0, 0], F32))
    assert res.score is None
    # min_points drops the single point and renumbers nothing else
    res = euclidean_clusters_host(xyz, lab, radius=0.2, min_points=2)
    assert res.instance.tolist() == [0, 1, 2, 2, 1, 0, -1] and res.count.tolist() == [2, 2, 2]
    # ignoring class 2 frees number 0 for the next component; nothing is ignored with ()
    res = euclidean_clusters_host(xyz, lab, radius=0.2, ignore_classes=(2, 0))
    assert res.instance.tolist() == [-1, 0, 1, 1, 0, -1, 2] and res.classes.tolist() == [1, 3, 1]
    lab0 = np.array([0, 0, 3, 3, 0, 0, -1])
    res = euclidean_clusters_host(xyz, lab0, radius=0.2)
    assert res.instance.tolist() == [-1, -1, 0, 0, -1, -1, -1]
    res = euclidean_clusters_host(xyz, lab0, radius=0.2, ignore_classes=())
    assert res.instance.tolist() == [0, 1, 2, 2, 1, 0, -1]
    # the centroid is the fixed-order float64 mean rounded once; the score follows the same rule
    sc = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7], F32)
    res = euclidean_clusters_host(xyz, lab, radius=0.2, scores=sc)
    assert res.centroid[0, 0] == F32((np.float64(xyz[0, 0]) + np.float64(xyz[5, 0])) / 2.0)
    assert res.score[0] == F32((np.float64(sc[0]) + np.float64(sc[5])) / 2.0) and res.score.dtype == F32


def test_empty_result_shapes_and_dtypes():
    from randlanet.utils.cluster import euclidean_clusters_host
    xyz = np.random.RandomState(0).uniform(0, 1, (50, 3))
    for kw in (dict(labels=np.zeros(50, np.int64)), dict(labels=np.full(50, -1)),
               dict(labels=np.arange(50) + 1, min_points=2, radius=1e-4)):
        kw.setdefault("radius", 0.5)
        res = euclidean_clusters_host(xyz, scores=np.ones(50), **kw)
        assert res.instance.dtype == np.int32 and (res.instance == -1).all()
        assert res.classes.shape == (0,) and res.classes.dtype == np.int64
        assert res.count.shape == (0,) and res.count.dtype == np.int32
        for a in (res.centroid, res.lo, res.hi):
            assert a.shape == (0, 3) and a.dtype == F32
        assert res.score.shape == (0,) and res.score.dtype == F32


def test_public_entry_on_the_cpu_is_the_twin():
    from randlanet.utils.cluster import euclidean_clusters
    xyz, lab, r, kw = ci.case("uniform_257")
    res = euclidean_clusters(xyz, lab, radius=r, scores=ci.scores_of("uniform_257"), device="cpu", **kw)
    ci.assert_same(res, ci.twin("uniform_257"))
    # float64 coordinates are converted to float32 first
    res = euclidean_clusters(xyz.astype(np.float64), lab, radius=r, scores=ci.scores_of("uniform_257"), device="cpu", **kw)
    ci.assert_same(res, ci.twin("uniform_257"))


# ------------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals():
    from randlanet.utils.cluster import euclidean_clusters, euclidean_clusters_host
    xyz = np.random.RandomState(1).uniform(0, 1, (10, 3)).astype(F32)
    lab = np.ones(10, np.int64)
    for fn in (euclidean_clusters_host, lambda *a, **k: euclidean_clusters(*a, device="cpu", **k)):
        with pytest.raises(ValueError, match=r"xyz has shape \(10, 2\), expected \(M, 3\)"):
            fn(xyz[:, :2], lab, radius=0.1)
        with pytest.raises(ValueError, match=r"xyz has shape \(30,\)"):
            fn(xyz.reshape(-1), lab, radius=0.1)
        with pytest.raises(ValueError, match=r"M=0 points"):
            fn(np.zeros((0, 3), F32), np.zeros(0, np.int64), radius=0.1)
        with pytest.raises(ValueError, match=r"labels have shape \(9,\)"):
            fn(xyz, lab[:9], radius=0.1)
        with pytest.raises(ValueError, match=r"labels have shape \(10,\) and dtype float64"):
            fn(xyz, lab.astype(np.float64), radius=0.1)
        with pytest.raises(ValueError, match=r"scores have shape \(10, 1\)"):
            fn(xyz, lab, radius=0.1, scores=np.ones((10, 1)))
        for bad in (np.nan, np.inf, -np.inf):
            x = xyz.copy()
            x[4, 1] = bad
            with pytest.raises(ValueError, match="non-finite coordinates, first at point 4"):
                fn(x, lab, radius=0.1)
        for bad in (0.0, -1.0, np.nan, np.inf, 1e30, 1e-50):          # (1e30 squared is not finite; 1e-50 is 0 in float32)
            with pytest.raises(ValueError, match="must be positive and finite"):
                fn(xyz, lab, radius=bad)
        for bad in (0, -3, 1.5):
            with pytest.raises(ValueError, match="min_points"):
                fn(xyz, lab, radius=0.1, min_points=bad)
        # an extent of 2^16 cells or more on an axis
        far = xyz.copy()
        far[3, 2] = 70000.0
        with pytest.raises(ValueError, match=r"reach 2\^16 = 65536 cells on an axis"):
            fn(far, lab, radius=1.0)
        assert fn(far, lab, radius=1.1).count.sum() == 10         # 70000 / (1.1 * 1.0625) < 2^16: accepted


# ------------------------------------------------------------------------------------------------ 4. scene_labels twin
def test_scene_labels_twin_ties_and_threshold():
    from randlanet.utils.cluster import scene_labels
    prob = np.array([[0.25, 0.5, 0.5, 0.0],         # a tie: the lowest class, confidence 0.5 / 1.25
                     [0.0, 0.0, 0.0, 2.0],          # un-normalised: confidence 1
                     [1.0, 1.0, 1.0, 1.0],          # all tied: class 0 at 0.25
                     [0.1, 0.2, 0.3, 0.4]], F32)
    lab, conf = scene_labels(prob)
    assert lab.tolist() == [1, 3, 0, 3] and lab.dtype == np.int64 and conf.dtype == F32
    assert conf[0] == F32(0.4) and conf[1] == 1 and conf[2] == F32(0.25)
    s = ((np.float64(prob[3, 0]) + np.float64(prob[3, 1])) + np.float64(prob[3, 2])) + np.float64(prob[3, 3])
    assert conf[3] == F32(np.float64(prob[3, 3]) / s)
    # the threshold is strict: a confidence equal to it keeps its label
    lab, conf2 = scene_labels(prob, min_confidence=0.4)
    assert lab.tolist() == [1, 3, -1, 3] and np.array_equal(conf, conf2)
    lab, _ = scene_labels(prob, min_confidence=float(np.nextafter(F32(0.4), F32(1))))
    assert lab[0] == -1 and lab[1] == 3 and lab[2] == -1
    lab, _ = scene_labels(prob, min_confidence=1.5)
    assert lab.tolist() == [-1] * 4
    # random rows against a per-row restatement
    rs = np.random.RandomState(3)
    prob = (rs.randint(0, 5, (500, 7)) / 4).astype(F32) + F32(0.125)
    lab, conf = scene_labels(prob, 0.3)
    for v in range(500):
        best = int(np.flatnonzero(prob[v] == prob[v].max())[0])
        s = np.float64(0)
        for c in range(7):
            s = s + np.float64(prob[v, c])
        want = F32(np.float64(prob[v, best]) / s)
        assert conf[v] == want and lab[v] == (best if want >= F32(0.3) else -1)


# --------------------------------------------------------------------------------------------------- 5. CPU-placed model
@pytest.fixture(scope="module")
def cpu_model():
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    return Model(RandLANetSettings(n_classes=4, n_points=1024, n_neighbors=8, layer_sizes=[8, 16, 32, 32]), use_gpu=False)


@pytest.mark.parametrize("mode", ["plain", "grid", "pad"])
def test_predict_instances_on_a_cpu_model_is_the_three_steps(cpu_model, mode):
    from randlanet._scene_path import VoteOptions
    from randlanet.utils import cluster as K
    from randlanet.utils import grid as G
    rs = np.random.RandomState(7)
    M = 600 if mode == "pad" else 3000
    xyz = rs.uniform(0, 6, (M, 3)).astype(F32)
    kw = dict(votes=1, batch_size=2, seed=2)
    radius, min_points, ignore, min_conf = 0.45, 2, (3,), 0.26
    cloud, inverse = xyz, None
    if mode == "grid":
        kw["grid"] = 0.3
        sub = G.grid_subsample_host(xyz, cell=0.3)
        cloud, inverse = sub.xyz, sub.inverse
        assert 1024 < cloud.shape[0] < M
    if mode == "pad":
        kw["pad_small_scenes"] = True
        assert M < cpu_model.settings.n_points
    np.random.seed(5)
    got = cpu_model.predict_instances(xyz, radius=radius, min_points=min_points, ignore_classes=ignore,
                                      min_confidence=min_conf, **kw)
    # the three steps on the un-normalised votes of the same crops
    np.random.seed(5)
    opt = VoteOptions(votes=1, batch_size=2, smooth=0.95, seed=2, grid=kw.get("grid"), pad=mode == "pad")
    prob, _, inv, V, *_ = cpu_model._scene_path.vote(xyz, None, opt, device_out=False)
    assert V == cloud.shape[0] and (inv is None) == (inverse is None)
    label, conf = K.scene_labels(prob, min_conf)
    want = K.euclidean_clusters_host(cloud, label, radius=radius, min_points=min_points, ignore_classes=ignore, scores=conf)
    if inverse is not None:
        assert np.array_equal(inv, inverse)
        label, want = label[inverse], want._replace(instance=want.instance[inverse])
    assert np.array_equal(got.label, label) and got.label.dtype == np.int64 and got.label.shape == (M,)
    ci.assert_same(got, want, mode)
    assert type(got).__name__ == "InstanceResult" and got._fields == ("instance", "label", "classes", "count", "centroid",
                                                                       "lo", "hi", "score")
    # and against predict_scene itself: the argmax of the normalised confidences is the label wherever it is not -1
    np.random.seed(5)
    out = cpu_model.predict_scene(xyz, **kw)
    top = np.sort(out, axis=0)
    clear = (got.label >= 0) & (top[-1] - top[-2] > 1e-6)
    assert clear.sum() > M // 2 and np.array_equal(out.argmax(0)[clear], got.label[clear])
    # something was found, something was left out, and ignored or unsure points are in no instance
    assert got.count.shape[0] >= 1 and (got.instance == -1).any()
    assert (got.instance[(got.label == 3) | (got.label == -1)] == -1).all()
    assert (got.classes != 3).all() and (got.count >= min_points).all()


def test_predict_instances_refuses_before_it_votes(cpu_model):
    xyz = np.random.RandomState(0).uniform(0, 5, (2000, 3)).astype(F32)
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError, match="radius"):
        cpu_model.predict_instances(xyz, radius=0.0)
    with pytest.raises(ValueError, match="min_points"):
        cpu_model.predict_instances(xyz, radius=0.5, min_points=0)
    bad = xyz.copy()
    bad[5, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        cpu_model.predict_instances(bad, radius=0.5)
    assert np.array_equal(np.random.get_state()[1], state)       # no forward ran: no permutation was drawn


# --------------------------------------------------------------------------------------------------------- 6. C ABI
def test_new_entries_are_exported_and_check_their_arguments_on_the_host():
    from randlanet import _hip
    names = ("rl_cluster_workspace_bytes", "rl_cluster_cells", "rl_cluster_union", "rl_cluster_reduce", "rl_scene_labels")
    for n in names:
        assert n in _hip.EXPORTS
    lib = _hip.lib()
    assert lib.rl_version() == _hip.ABI_VERSION == 110
    M = 5000
    need = lib.rl_cluster_workspace_bytes(M)
    assert need > 60 * M and lib.rl_cluster_workspace_bytes(0) == 0 and lib.rl_cluster_workspace_bytes(2 ** 31 - 1) == 0
    fake = 1 << 20              # never dereferenced: every call below is refused before a launch
    E = _hip.ERR_ARGS
    assert lib.rl_cluster_cells(fake, M, 0.0, fake, fake, need, None) == E
    assert b"rl_cluster_cells: radius=0 must be positive and finite" in lib.rl_last_error()
    assert lib.rl_cluster_cells(fake, M, float("inf"), fake, fake, need, None) == E
    assert lib.rl_cluster_cells(fake, 0, 0.5, fake, fake, need, None) == E
    assert lib.rl_cluster_cells(fake, M, 0.5, fake, fake, need - 1, None) == E
    assert b"workspace" in lib.rl_last_error()
    assert lib.rl_cluster_cells(fake, M, 0.5, fake, fake + 8, need, None) == E
    assert b"aligned" in lib.rl_last_error()
    assert lib.rl_cluster_cells(None, M, 0.5, fake, fake, need, None) == E
    assert lib.rl_cluster_union(fake, fake, M, 0.5, None, 0, 10, 0, fake, fake, fake, need, None) == E
    assert b"min_points=0" in lib.rl_last_error()
    assert lib.rl_cluster_union(fake, fake, M, 0.5, None, 1, 10, 1, fake, fake, fake, need, None) == E
    assert b"ignored classes" in lib.rl_last_error()
    assert lib.rl_cluster_union(fake, fake, M, 0.5, None, 0, 50, 1, fake, fake, fake, need, None) == E
    assert b"key_bits=50" in lib.rl_last_error()
    assert lib.rl_cluster_union(fake, fake, M, -1.0, None, 0, 10, 1, fake, fake, fake, need, None) == E
    assert lib.rl_cluster_union(fake, None, M, 0.5, None, 0, 10, 1, fake, fake, fake, need, None) == E
    assert lib.rl_cluster_reduce(fake, fake, None, M, 0, fake, fake, fake, fake, fake, None, fake, need, None) == E
    assert b"I=0 instances" in lib.rl_last_error()
    assert lib.rl_cluster_reduce(fake, fake, fake, M, 3, fake, fake, fake, fake, fake, None, fake, need, None) == E
    assert b"go together" in lib.rl_last_error()
    assert lib.rl_cluster_reduce(fake, fake, None, M, M + 1, fake, fake, fake, fake, fake, None, fake, need, None) == E
    assert lib.rl_scene_labels(fake, 0, 3, 0.0, fake, fake, None) == E
    assert lib.rl_scene_labels(fake, 10, 0, 0.0, fake, fake, None) == E
    assert lib.rl_scene_labels(fake, 10, 3, float("nan"), fake, fake, None) == E
    assert lib.rl_scene_labels(fake, 10, 3, 0.0, None, fake, None) == E
