"""Smoothness-constrained clustering on the MI355X: rl_cluster_union_smooth (csrc/cluster.hip) against the numpy twin
(utils/cluster.py with normals and normal_angle) on every case of tests/smooth_inputs.py, bit for bit on every array, with and
without curvature and scores; Model.predict_instances(normal_angle=...) and Model.evaluate_instances(normal_angle=...) on a
GPU-placed model against the twins run on that model's own voted probabilities and its own device-estimated normals."""
import math

import numpy as np
import pytest
import torch

import cluster_inputs as ci
import smooth_inputs as sm
from smooth_twin import twin

pytestmark = pytest.mark.gpu
F32 = np.float32


def _dev():
    return torch.device("cuda", 0)


@pytest.mark.parametrize("name", sm.CASES)
def test_device_equals_the_twin(name):
    from randlanet.utils.cluster import euclidean_clusters
    xyz, lab, r, kw = sm.case(name)
    res = euclidean_clusters(xyz, lab, radius=r, scores=sm.scores_of(name), device=_dev(), **kw)
    sm.assert_same(res, twin(name), name)


@pytest.mark.parametrize("name", ["corner", "crease_cut", "curv:uniform_4097", "dense:uniform_20000_min5"])
def test_without_scores_and_the_curvature_on_and_off(name):
    from randlanet import _hip
    from randlanet.utils.cluster import euclidean_clusters, euclidean_clusters_host
    xyz, lab, r, kw = sm.case(name)
    res = euclidean_clusters(xyz, lab, radius=r, **kw)               # device=None: a GPU is available
    assert _hip.lib().rl_last_kernel() == b"cl_reduce"
    assert res.score is None
    sm.assert_same(res, twin(name)._replace(score=None), name)
    # the same cloud with the curvature taken away or put on: another answer, the twin's again
    kw = dict(kw)
    if "curvature" in kw:
        del kw["curvature"], kw["max_curvature"]
    else:
        kw.update(curvature=np.random.RandomState(3).uniform(0, 1, xyz.shape[0]).astype(F32), max_curvature=0.75)
    want = euclidean_clusters_host(xyz, lab, radius=r, **kw)
    got = euclidean_clusters(xyz, lab, radius=r, device="cuda", **kw)
    sm.assert_same(got, want, name)
    assert not np.array_equal(want.instance, twin(name).instance)


def test_nothing_kept_and_a_smaller_cloud_after_a_larger_one():
    """min_points above every component: nothing is reduced; the cached workspace serves a smaller cloud after a larger one."""
    from randlanet.utils.cluster import euclidean_clusters
    xyz, lab, r, kw = sm.case("dense:uniform_20000")
    res = euclidean_clusters(xyz, lab, radius=r, device=_dev(), scores=sm.scores_of("dense:uniform_20000"),
                             **dict(kw, min_points=4000))
    assert (res.instance == -1).all() and res.instance.dtype == np.int32
    assert res.classes.shape == (0,) and res.count.shape == (0,) and res.centroid.shape == (0, 3) and res.score.shape == (0,)
    for name in ("threshold", "ring_10", "corner"):
        xyz, lab, r, kw = sm.case(name)
        sm.assert_same(euclidean_clusters(xyz, lab, radius=r, scores=sm.scores_of(name), device=_dev(), **kw), twin(name))


def test_many_ignored_classes_and_wide_labels():
    """Labels that agree in their low 32 bits only are different classes; 40 ignored classes."""
    from randlanet.utils.cluster import euclidean_clusters, euclidean_clusters_host
    xyz, lab, r, kw = sm.case("curv:uniform_4097")
    lab = lab.copy()
    lab[(lab == 2) & (np.arange(lab.shape[0]) % 2 == 0)] = 2 + (1 << 32)      # half of class 2: the same low 32 bits
    lab[::5] = 100 + np.arange(lab[::5].shape[0]) % 40
    kw = dict(kw, ignore_classes=tuple(range(100, 140)) + (0,))
    want = euclidean_clusters_host(xyz, lab, radius=r, **kw)
    got = euclidean_clusters(xyz, lab, radius=r, device=_dev(), **kw)
    sm.assert_same(got, want)
    assert (2 + (1 << 32)) in want.classes and 2 in want.classes and want.count.max() > 3
    # with the two taken for one class the answer is another one: the case does hold pairs that only the high bits part
    same = euclidean_clusters_host(xyz, np.where(lab == 2 + (1 << 32), 2, lab), radius=r, **kw)
    assert not np.array_equal(same.instance, want.instance)


def test_too_fine_a_grid_is_refused_from_the_device_dims():
    from randlanet.utils.cluster import euclidean_clusters
    xyz = np.array([[0, 0, 0], [0, 70000, 0], [1, 2, 3]], F32)
    nrm = np.tile(np.array([0, 1, 0], F32), (3, 1))
    with pytest.raises(ValueError, match=r"reach 2\^16 = 65536 cells on an axis"):
        euclidean_clusters(xyz, np.ones(3, np.int64), radius=1.0, device=_dev(), normals=nrm, normal_angle=20)
    res = euclidean_clusters(xyz, np.ones(3, np.int64), radius=1.1, device=_dev(), normals=nrm, normal_angle=20)
    assert res.count.tolist() == [1, 1, 1]


# --------------------------------------------------------------------------------------------------------- Model
@pytest.fixture(scope="module", params=[None, 16], ids=["estimated", "appended"])
def gpu_model(request):
    """(a GPU-placed model, the `normals` keyword it is made for)"""
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    model = Model(RandLANetSettings(n_classes=4, n_points=2048, n_neighbors=8, layer_sizes=[16, 32],
                                    n_features=4 if request.param else 0), use_gpu=True)
    assert model.device.type == "cuda"
    return model, request.param


def _room(rs, M):
    """A floor and two walls of 5 x 5 that meet in creases, sampled at random, with a little noise."""
    xyz = rs.uniform(0, 5, (M, 3))
    xyz[np.arange(M), 2 - rs.randint(0, 3, M)] = 0.0
    return (xyz + rs.normal(0, 0.003, (M, 3))).astype(F32)


VIEW = (2.5, 2.5, 2.5)


def _by_the_twins(model, normals, xyz, grid, radius, min_points, ignore, min_conf, angle, top, k):
    """predict_instances(normal_angle=angle, max_curvature=top, cluster_normals=k, oriented_boxes=True) step by step: the
    model's own votes and device-estimated normals, then the numpy twins.  Returns (label, ClusterResult, BoxResult or None,
    the curvature of the clustered cloud, inverse or None)."""
    from randlanet import _ops as ops
    from randlanet._scene_path import VoteOptions
    from randlanet.utils import boxes as B
    from randlanet.utils import cluster as K
    opt = VoteOptions(votes=1, batch_size=4, smooth=0.95, seed=2, grid=grid, normals=normals, viewpoint=VIEW)
    prob, _, inverse, V, cloud, *_ = model._scene_path.vote(xyz, None, opt, device_out=True)
    assert prob.is_cuda and (grid is None) == (inverse is None)
    with torch.cuda.device(model.device):
        cloud = cloud if torch.is_tensor(cloud) else torch.from_numpy(cloud).to(model.device)
        if normals is None:
            assert cloud.shape[1] == 3
            nrm, curv = ops.estimate_normals(cloud[:, :3].contiguous(), k, VIEW)
        else:
            assert cloud.shape[1] == 7
            nrm, curv = cloud[:, 3:6], cloud[:, 6]
    cloud, nrm, curv = cloud.cpu().numpy(), nrm.cpu().numpy(), curv.cpu().numpy()
    label, conf = K.scene_labels(prob.cpu().numpy(), min_conf)
    extra = dict(curvature=curv, max_curvature=top) if top is not None else {}
    res = K.euclidean_clusters_host(cloud[:, :3], label, radius=radius, min_points=min_points, ignore_classes=ignore,
                                    scores=conf, normals=nrm, normal_angle=angle, **extra)
    if inverse is not None:
        inverse = inverse.cpu().numpy()
        label, res = label[inverse], res._replace(instance=res.instance[inverse])
    box = B.instance_boxes_host(xyz, res.instance, res.count.shape[0]) if res.count.shape[0] else None
    return label, res, box, curv, inverse


@pytest.mark.parametrize("grid", [None, 0.1])
def test_predict_instances_is_the_twins_on_its_own_votes_and_normals(gpu_model, grid):
    model, normals = gpu_model
    xyz = _room(np.random.RandomState(11), 12000)
    radius, min_points, ignore, min_conf, angle, top, k = 0.2, 3, (), 0.0, 8.0, 0.03, 12
    kw = dict(radius=radius, min_points=min_points, ignore_classes=ignore, min_confidence=min_conf, votes=1, batch_size=4,
              seed=2, grid=grid, normals=normals, viewpoint=VIEW)
    for max_curvature in (None, top):
        np.random.seed(5)
        got = model.predict_instances(xyz, oriented_boxes=True, normal_angle=angle, max_curvature=max_curvature,
                                      cluster_normals=k, **kw)
        np.random.seed(5)
        label, want, box, curv, inverse = _by_the_twins(model, normals, xyz, grid, radius, min_points, ignore, min_conf,
                                                        angle, max_curvature, k)
        assert type(got).__name__ == "OrientedInstanceResult"
        assert got.label.shape == (12000,) and np.array_equal(got.label, label)
        ci.assert_same(got, want, f"grid={grid} max_curvature={max_curvature}")
        I = want.count.shape[0]
        assert I >= 2 and box is not None
        for f in ("center", "axes", "extent", "eigenvalues"):
            a, b = getattr(got, "box_" + f), getattr(box, f)
            assert a.dtype == b.dtype and np.array_equal(a, b), f
        if max_curvature is not None:               # the points on the creases were cut
            cut = curv > F32(top)
            cut = cut if inverse is None else cut[inverse]
            assert cut.sum() > 100 and (got.instance[cut] == -1).all()
        # the rule did something: not the plain answer
        np.random.seed(5)
        plain = model.predict_instances(xyz, **kw)
        assert not np.array_equal(plain.instance, got.instance)
        print(f"predict_instances grid={grid} normals={normals} max_curvature={max_curvature}: {I} instances, the largest "
              f"of {int(want.count.max())}; plain {plain.count.shape[0]}, the largest of {int(plain.count.max())}")


def test_evaluate_instances_is_the_evaluator_fed_by_the_twins(gpu_model):
    from randlanet.utils.instance_metrics import InstanceEvaluator
    model, normals = gpu_model
    rs = np.random.RandomState(13)
    scenes = []
    for M in (9000, 7000):
        xyz = _room(rs, M)
        face = np.argmin(np.abs(xyz), axis=1)                   # the annotation: every face is an object of its own class
        ids = face.astype(np.int64) * 3
        ids[xyz.max(axis=1) > 4.9] = -1
        scenes.append((xyz, None, (face + 1).astype(np.int64), ids))
    radius, min_points, ignore, min_conf, angle, top, k = 0.25, 3, (), 0.0, 8.0, 0.03, 12
    kw = dict(radius=radius, min_points=min_points, ignore_classes=ignore, min_confidence=min_conf, votes=1, batch_size=4,
              seed=2, normals=normals, viewpoint=VIEW, normal_angle=angle, max_curvature=top, cluster_normals=k)
    np.random.seed(5)
    got = model.evaluate_instances(scenes, min_gt_points=50, **kw)
    np.random.seed(5)
    ev = InstanceEvaluator(4, ignore_classes=ignore, min_gt_points=50, device="cpu")
    n_pred = 0
    for xyz, _, labels, ids in scenes:
        _, res, _, _, _ = _by_the_twins(model, normals, xyz, None, radius, min_points, ignore, min_conf, angle, top, k)
        ev.add(res.instance, res.classes, res.score, ids, labels)
        n_pred += res.count.shape[0]
    want = ev.result()
    assert list(got.keys()) == list(want.keys())
    for key in got:
        g, w = got[key], want[key]
        assert (g == w) or (isinstance(g, float) and math.isnan(g) and math.isnan(w)), (key, g, w)
    assert sum(got[f"class {c} n_pred"] for c in range(4)) == n_pred and n_pred >= 2
    assert sum(got[f"class {c} n_gt"] for c in range(4)) == 6
    print(f"evaluate_instances normals={normals}: {n_pred} predictions, AP25 {got['AP25']}, mCov {got['mCov']}")
