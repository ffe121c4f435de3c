"""Euclidean clustering on the MI355X: csrc/cluster.hip against the numpy twin (utils/cluster.py) on every case of
tests/cluster_inputs.py, bit for bit on every array; rl_scene_labels against its twin; Model.predict_instances on a GPU-placed
model against the three steps - votes, labels twin, clustering twin - run on that model's own voted probabilities."""
import numpy as np
import pytest
import torch

import cluster_inputs as ci

pytestmark = pytest.mark.gpu
F32 = np.float32


def _dev():
    return torch.device("cuda", 0)


@pytest.mark.parametrize("name", ci.CASES)
def test_device_equals_the_twin(name):
    from randlanet.utils.cluster import euclidean_clusters
    xyz, lab, r, kw = ci.case(name)
    res = euclidean_clusters(xyz, lab, radius=r, scores=ci.scores_of(name), device=_dev(), **kw)
    ci.assert_same(res, ci.twin(name), name)


def test_without_scores_and_default_device():
    from randlanet import _hip
    from randlanet.utils.cluster import euclidean_clusters
    xyz, lab, r, kw = ci.case("uniform_4097")
    res = euclidean_clusters(xyz, lab, radius=r, **kw)               # device=None: a GPU is available
    assert _hip.lib().rl_last_kernel() == b"cl_reduce"
    assert res.score is None
    ci.assert_same(res, ci.twin("uniform_4097")._replace(score=None))
    # min_points above every component: nothing is kept, nothing is reduced
    res = euclidean_clusters(xyz, lab, radius=r, min_points=100, scores=ci.scores_of("uniform_4097"), device="cuda")
    assert (res.instance == -1).all() and res.instance.dtype == np.int32
    assert res.classes.shape == (0,) and res.classes.dtype == np.int64 and res.count.shape == (0,)
    assert res.centroid.shape == res.lo.shape == res.hi.shape == (0, 3) and res.score.shape == (0,)
    assert res.centroid.dtype == res.score.dtype == F32 and res.count.dtype == np.int32


def test_many_ignored_classes_and_wide_labels():
    """Labels that agree in their low 32 bits only are different classes; 40 ignored classes."""
    from randlanet.utils.cluster import euclidean_clusters, euclidean_clusters_host
    xyz, lab, r, _ = ci.case("uniform_4097")
    lab = lab.copy()
    lab[lab == 2] = 2 + (1 << 32)
    lab[::5] = 100 + np.arange(lab[::5].shape[0]) % 40
    ignore = tuple(range(100, 140)) + (0,)
    want = euclidean_clusters_host(xyz, lab, radius=2 * r, ignore_classes=ignore)
    got = euclidean_clusters(xyz, lab, radius=2 * r, ignore_classes=ignore, device=_dev())
    ci.assert_same(got, want)
    assert (2 + (1 << 32)) in want.classes and want.count.max() > 3


def test_too_fine_a_grid_is_refused_from_the_device_dims():
    from randlanet.utils.cluster import euclidean_clusters
    xyz = np.array([[0, 0, 0], [0, 70000, 0], [1, 2, 3]], F32)
    with pytest.raises(ValueError, match=r"reach 2\^16 = 65536 cells on an axis"):
        euclidean_clusters(xyz, np.ones(3, np.int64), radius=1.0, device=_dev())
    res = euclidean_clusters(xyz, np.ones(3, np.int64), radius=1.1, device=_dev())
    assert res.count.tolist() == [1, 1, 1]


@pytest.mark.parametrize("C", [1, 5, 40])
def test_scene_labels_equals_the_twin(C):
    from randlanet import _ops as ops
    from randlanet.utils.cluster import scene_labels
    rs = np.random.RandomState(C)
    V = 70001
    prob = (rs.randint(0, 4, (V, C)) / 4).astype(F32) + F32(0.125)      # quantised: many ties for the argmax
    prob[::7] = rs.uniform(0, 3, prob[::7].shape).astype(F32)
    dropped = kept = False
    for min_conf in (0.0, 0.3, 1.0 / C):
        want_l, want_c = scene_labels(prob, min_conf)
        with torch.cuda.device(_dev()):
            lab, conf = ops.scene_labels(torch.from_numpy(prob).to(_dev()), min_conf)
        assert lab.dtype == torch.int64 and conf.dtype == torch.float32
        assert np.array_equal(conf.cpu().numpy(), want_c) and np.array_equal(lab.cpu().numpy(), want_l)
        dropped, kept = dropped or bool((want_l == -1).any()), kept or bool((want_l >= 0).any())
    assert kept and (C == 1 or dropped)                           # some threshold dropped labels, some kept them


# --------------------------------------------------------------------------------------------------------- Model
@pytest.fixture(scope="module")
def gpu_model():
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    model = Model(RandLANetSettings(n_classes=4, n_points=2048, n_neighbors=8, layer_sizes=[16, 32]), use_gpu=True)
    assert model.device.type == "cuda"
    return model


@pytest.mark.parametrize("grid", [None, 0.25])
def test_predict_instances_is_the_three_steps_on_its_own_votes(gpu_model, grid):
    from randlanet._scene_path import VoteOptions
    from randlanet.utils import cluster as K
    rs = np.random.RandomState(11)
    M = 12000
    xyz = rs.uniform(0, 5, (M, 3)).astype(F32)
    # without grid every point takes part (at 96 points per unit volume and r = 0.2 a point has 3.2 neighbours: instances
    # exist whatever the untrained network answers); with grid class 0 is ignored and unsure points are dropped
    radius, min_points = 0.2, 3
    ignore, min_conf = ((), 0.0) if grid is None else ((0,), 0.26)
    kw = dict(votes=1, batch_size=4, seed=2, grid=grid)
    np.random.seed(5)
    got = gpu_model.predict_instances(xyz, radius=radius, min_points=min_points, ignore_classes=ignore,
                                      min_confidence=min_conf, **kw)
    np.random.seed(5)
    opt = VoteOptions(votes=1, batch_size=4, smooth=0.95, seed=2, grid=grid)
    prob, _, inverse, V, cloud, *_ = gpu_model._scene_path.vote(xyz, None, opt, device_out=True)
    assert prob.is_cuda
    cloud = cloud.cpu().numpy() if torch.is_tensor(cloud) else cloud
    label, conf = K.scene_labels(prob.cpu().numpy(), min_conf)
    want = K.euclidean_clusters_host(cloud[:, :3], label, radius=radius, min_points=min_points, ignore_classes=ignore,
                                     scores=conf)
    if grid is not None:
        inv = inverse.cpu().numpy()
        assert 2048 < V < M and inv.shape == (M,)
        label, want = label[inv], want._replace(instance=want.instance[inv])
    else:
        assert inverse is None and V == M
    assert got.label.shape == (M,) and got.label.dtype == np.int64 and np.array_equal(got.label, label)
    ci.assert_same(got, want, f"grid={grid}")
    # well-formed: instances 0 .. I-1, members of one class that takes part, counts over what was clustered
    I = got.count.shape[0]
    print(f"predict_instances grid={grid}: {I} instances, labels {np.bincount(got.label + 1, minlength=5).tolist()} (-1 .. 3)")
    assert got.instance.dtype == np.int32 and got.instance.max(initial=-1) == I - 1
    assert I >= 1 or grid is not None
    assert (got.count >= min_points).all() and (got.classes >= 0).all() and not np.isin(got.classes, ignore).any()
    inside = got.instance >= 0
    assert np.array_equal(got.label[inside], got.classes[got.instance[inside]])
    if grid is None:
        assert np.array_equal(np.bincount(got.instance[inside], minlength=I), got.count)
    else:
        assert (np.bincount(got.instance[inside], minlength=I) >= got.count).all()
    assert (got.lo <= got.centroid).all() and (got.centroid <= got.hi).all()
    assert ((got.score >= F32(min_conf)) & (got.score <= 1)).all()
