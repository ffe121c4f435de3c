"""DBSCAN's density rule (min_samples) on the MI355X: rl_cluster_union_dense (csrc/cluster.hip) against the numpy twin
(utils/cluster.py) on every case of tests/dbscan_inputs.py, bit for bit on every array, with and without scores; min_samples =
1 against the path as it was, launches included; the refusals; Model.predict_instances(min_samples=3) on a GPU-placed model
against the three steps - votes, labels twin, clustering twin - run on that model's own voted probabilities."""
import numpy as np
import pytest
import torch

import cluster_inputs as ci
import dbscan_inputs as di

pytestmark = pytest.mark.gpu
F32 = np.float32


def _dev():
    return torch.device("cuda", 0)


@pytest.mark.parametrize("name", di.CASES)
def test_device_equals_the_twin(name):
    from randlanet import _hip
    from randlanet.utils.cluster import euclidean_clusters
    xyz, lab, kw = di.case(name)
    want = di.twin(name)
    res = euclidean_clusters(xyz, lab, scores=di.scores_of(name), device=_dev(), **kw)
    ci.assert_same(res, want, name)
    res = euclidean_clusters(xyz, lab, device=_dev(), **kw)
    assert res.score is None
    ci.assert_same(res, want._replace(score=None), name + " without scores")
    assert _hip.lib().rl_last_kernel() == (b"cl_reduce" if want.count.shape[0] else b"cl_finish")


@pytest.mark.parametrize("name", ["uniform_4097", "uniform_20000_min5", "chain_3000_cut", "duplicates"])
def test_min_samples_1_is_the_path_as_it_was(name):
    """The same arrays, the same number of launches as without the keyword, the last kernel cl_reduce; min_samples = 2 on the
    same cloud launches two kernels more (support and attach)."""
    from randlanet import _hip
    from randlanet.utils.cluster import euclidean_clusters
    lib = _hip.lib()
    xyz, lab, r, kw = ci.case(name)
    sc = ci.scores_of(name)
    euclidean_clusters(xyz, lab, radius=r, scores=sc, device=_dev(), **kw)         # (workspaces and modules are there now)
    n0 = lib.rl_launch_count()
    plain = euclidean_clusters(xyz, lab, radius=r, scores=sc, device=_dev(), **kw)
    n1 = lib.rl_launch_count()
    one = euclidean_clusters(xyz, lab, radius=r, scores=sc, device=_dev(), min_samples=1, **kw)
    n2 = lib.rl_launch_count()
    assert lib.rl_last_kernel() == b"cl_reduce"
    ci.assert_same(one, plain, name)
    ci.assert_same(one, ci.twin(name), name)
    assert n2 - n1 == n1 - n0 > 0
    two = euclidean_clusters(xyz, lab, radius=r, scores=sc, device=_dev(), min_samples=2, **kw)
    n3 = lib.rl_launch_count()
    assert n3 - n2 == n1 - n0 + 2 or two.count.shape[0] == 0


def test_min_samples_1_with_normals_is_the_smooth_path_as_it_was():
    from randlanet import _hip
    from randlanet.utils.cluster import euclidean_clusters, euclidean_clusters_host
    xyz, lab, kw = di.case("smooth_dense_curv_ms4")
    kw = dict(kw, min_samples=1)
    want = euclidean_clusters_host(xyz, lab, **kw)
    lib = _hip.lib()
    n0 = lib.rl_launch_count()
    plain = euclidean_clusters(xyz, lab, device=_dev(), **{k: v for k, v in kw.items() if k != "min_samples"})
    n1 = lib.rl_launch_count()
    one = euclidean_clusters(xyz, lab, device=_dev(), **kw)
    n2 = lib.rl_launch_count()
    assert lib.rl_last_kernel() == b"cl_reduce" and n2 - n1 == n1 - n0
    ci.assert_same(one, want)
    ci.assert_same(plain, want)


def test_refusals():
    from randlanet import _hip
    from randlanet.utils.cluster import euclidean_clusters
    xyz, lab, _ = di.case("border_tie_ms4")
    for bad in (0, -3, 2.5, None, float("nan")):
        with pytest.raises(ValueError, match="min_samples"):
            euclidean_clusters(xyz, lab, radius=0.25, min_samples=bad, device=_dev())
    # the C entry itself: RL_ERR_ARGS before any launch
    lib = _hip.lib()
    dev = _dev()
    M = xyz.shape[0]
    with torch.cuda.device(dev):
        x, l = torch.from_numpy(xyz).to(dev), torch.from_numpy(lab).to(dev)
        need = int(lib.rl_cluster_dense_workspace_bytes(M, 0))
        assert need >= int(lib.rl_cluster_workspace_bytes(M)) + 8 * M
        assert int(lib.rl_cluster_dense_workspace_bytes(M, 1)) >= int(lib.rl_cluster_smooth_workspace_bytes(M)) + 8 * M
        assert int(lib.rl_cluster_dense_workspace_bytes(0, 0)) == 0
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        head = torch.zeros(4, dtype=torch.int64, device=dev)
        inst = torch.empty(M, dtype=torch.int32, device=dev)
        _hip.check(lib.rl_cluster_cells(x.data_ptr(), M, 0.25, head.data_ptr(), ws.data_ptr(), ws.numel(), None),
                   "rl_cluster_cells")
        torch.cuda.synchronize()

        def call(min_samples, nbytes=need, curvature=None):
            return lib.rl_cluster_union_dense(x.data_ptr(), l.data_ptr(), M, 0.25, None, 0, 3, 1, None, curvature, 0.0, 0.0,
                                              min_samples, inst.data_ptr(), head[3:].data_ptr(), ws.data_ptr(), nbytes, None)
        n0 = lib.rl_launch_count()
        assert call(0) == _hip.ERR_ARGS and call(-1) == _hip.ERR_ARGS
        assert call(2, nbytes=int(lib.rl_cluster_workspace_bytes(M))) == _hip.ERR_ARGS      # the plain workspace is too small
        assert call(2, curvature=x.data_ptr()) == _hip.ERR_ARGS                            # curvature without normals
        assert lib.rl_launch_count() == n0


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
    # the sizes of test_cluster_gpu.py: without grid every point takes part (96 points per unit volume, r = 0.2: 3.2
    # neighbours, so core, border and noise points exist at min_samples = 3 whatever the untrained network answers); with
    # grid class 0 is ignored and unsure points are dropped
    radius, min_points = 0.2, 3
    ignore, min_conf = ((), 0.0) if grid is None else ((0,), 0.26)
    kw = dict(votes=1, batch_size=4, seed=2, grid=grid)
    np.random.seed(5)
    got = gpu_model.predict_instances(xyz, radius=radius, min_points=min_points, ignore_classes=ignore,
                                      min_confidence=min_conf, min_samples=3, **kw)
    np.random.seed(5)
    opt = VoteOptions(votes=1, batch_size=4, smooth=0.95, seed=2, grid=grid)
    prob, _, inverse, V, cloud, *_ = gpu_model._scene_path.vote(xyz, None, opt, device_out=True)
    cloud = cloud.cpu().numpy() if torch.is_tensor(cloud) else cloud
    label, conf = K.scene_labels(prob.cpu().numpy(), min_conf)
    want = K.euclidean_clusters_host(cloud[:, :3], label, radius=radius, min_points=min_points, ignore_classes=ignore,
                                     scores=conf, min_samples=3)
    plain = K.euclidean_clusters_host(cloud[:, :3], label, radius=radius, min_points=min_points, ignore_classes=ignore,
                                      scores=conf)
    if grid is not None:
        inv = inverse.cpu().numpy()
        label, want = label[inv], want._replace(instance=want.instance[inv])
        plain = plain._replace(instance=plain.instance[inv])
    assert np.array_equal(got.label, label)
    ci.assert_same(got, want, f"grid={grid}")
    print(f"predict_instances(min_samples=3) grid={grid}: {got.count.shape[0]} instances, {plain.count.shape[0]} at 1")
    if grid is None:
        assert got.count.shape[0] >= 1 and not np.array_equal(got.instance, plain.instance)
    # evaluate_instances takes the keyword too, and a bad one is refused before any vote
    with pytest.raises(ValueError, match="min_samples"):
        gpu_model.predict_instances(xyz, radius=radius, min_samples=0)
    with pytest.raises(ValueError, match="min_samples"):
        gpu_model.evaluate_instances([(xyz, None, np.zeros(M, np.int64), np.zeros(M, np.int64))], radius=radius,
                                     min_samples=1.5)
