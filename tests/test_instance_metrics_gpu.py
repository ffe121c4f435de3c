"""Instance evaluation on the MI355X: csrc/pairs.hip against the numpy twin (utils/instance_metrics.py) on every case of
tests/pairs_inputs.py, exactly; the range flag; InstanceEvaluator on the device against the same evaluator on the host; and
Model.evaluate_instances on a GPU-placed model against the steps run by hand on that model's own predict_instances output."""
import math

import numpy as np
import pytest
import torch

import pairs_inputs as pi

pytestmark = pytest.mark.gpu
F32 = np.float32


def _dev():
    return torch.device("cuda", 0)


def same_result(got, want):
    assert list(got.keys()) == list(want.keys())
    for k in got:
        g, w = got[k], want[k]
        assert (g == w) or (isinstance(g, float) and math.isnan(g) and math.isnan(w)), (k, g, w)


@pytest.mark.parametrize("name", pi.CASES)
def test_device_equals_the_twin(name):
    from randlanet.utils.instance_metrics import pair_counts
    got = pair_counts(*pi.case(name), device=_dev())
    pi.assert_same(got, pi.twin(name), name)
    assert got[2].sum() == pi.case(name)[0].shape[0]


def test_default_device_last_kernel_and_device_tensors():
    from randlanet import _hip
    from randlanet import _ops as ops
    from randlanet.utils.instance_metrics import pair_counts
    a, b, A, B = pi.case("m_4097")
    got = pair_counts(a, b, A, B)                                    # device=None: a GPU is available
    assert _hip.lib().rl_last_kernel() == b"pr_counts"
    pi.assert_same(got, pi.twin("m_4097"))
    # device tensors in, device tensors out; int32 and int64 ids in either place
    for ta, tb in ((torch.int32, torch.int64), (torch.int64, torch.int32)):
        with torch.cuda.device(_dev()):
            res = ops.pair_counts(torch.from_numpy(a).to(_dev(), ta), torch.from_numpy(b).to(_dev(), tb), A, B)
        assert all(t.is_cuda for t in res)
        assert [t.dtype for t in res] == [torch.int32, torch.int32, torch.int64]
        pi.assert_same(tuple(t.cpu().numpy() for t in res), pi.twin("m_4097"))


def test_a_value_out_of_range_raises_from_the_flag():
    from randlanet.utils.instance_metrics import pair_counts
    a, b, A, B = pi.case("m_70001")
    for where in (0, 2048, 70000):                                   # the first chunk, a later one, the last position
        bad = a.copy()
        bad[where] = A
        with pytest.raises(ValueError, match="out of range"):
            pair_counts(bad, b, A, B, device=_dev())
        bad = b.copy()
        bad[where] = B + 5
        with pytest.raises(ValueError, match="out of range"):
            pair_counts(a, bad, A, B, device=_dev())
    pi.assert_same(pair_counts(a, b, A, B, device=_dev()), pi.twin("m_70001"))       # and the flag is lowered again


# ----------------------------------------------------------------------------------------------------- InstanceEvaluator
def blob_scene(M=70001, n_obj=40, seed=3):
    """About 40 ground-truth objects as noisy blobs over a floor of class 0, ids with gaps; predictions by Euclidean
    clustering of labels of which one in twenty is wrong."""
    from randlanet.utils.cluster import euclidean_clusters
    rs = np.random.RandomState(seed)
    centres = np.stack([rs.uniform(0, 30, n_obj), rs.uniform(0, 30, n_obj), rs.uniform(1, 2, n_obj)], axis=1)
    owner = rs.randint(-1, n_obj, M)                                 # -1: the floor
    xyz = np.where(owner[:, None] >= 0, centres[np.maximum(owner, 0)] + rs.normal(0, 0.35, (M, 3)),
                   np.stack([rs.uniform(0, 30, M), rs.uniform(0, 30, M), rs.uniform(0, 0.1, M)], axis=1)).astype(F32)
    gt_ids = np.where(owner >= 0, owner * 3 + 1, -1).astype(np.int64)
    gt_labels = np.where(owner >= 0, 1 + owner % 3, 0).astype(np.int64)
    noisy = gt_labels.copy()
    flip = rs.rand(M) < 0.05
    noisy[flip] = rs.randint(0, 4, int(flip.sum()))
    res = euclidean_clusters(xyz, noisy, radius=0.12, min_points=15, scores=rs.rand(M).astype(F32), device=_dev())
    return res, gt_ids, gt_labels


def test_evaluator_on_the_device_equals_the_host():
    from randlanet.utils.instance_metrics import InstanceEvaluator
    res, gt_ids, gt_labels = blob_scene()
    assert res.count.shape[0] >= 30
    out = []
    for device, as_tensor in (("cpu", False), (_dev(), False), (_dev(), True)):
        ev = InstanceEvaluator(4, min_gt_points=100, device=device)
        inst = torch.from_numpy(res.instance).to(_dev()) if as_tensor else res.instance
        ev.add(inst, res.classes, res.score, gt_ids, gt_labels)
        out.append(ev.result())
    same_result(out[1], out[0])
    same_result(out[2], out[0])
    r = out[0]
    print({k: r[k] for k in ("AP", "AP50", "AP25", "mCov", "mWCov")})
    assert r["class 1 n_gt"] + r["class 2 n_gt"] + r["class 3 n_gt"] == 40
    assert 0.0 < r["AP25"] <= 1.0 and 0.0 < r["mCov"] < 1.0


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
def test_evaluate_instances_is_the_steps_by_hand_on_its_own_predictions(gpu_model, grid):
    from randlanet.utils.instance_metrics import InstanceEvaluator
    rs = np.random.RandomState(11)
    scenes = []
    for M in (12000, 9000):
        xyz = rs.uniform(0, 5, (M, 3)).astype(F32)
        ids = (np.floor(xyz[:, 0] / 2.5) + 2 * np.floor(xyz[:, 1] / 2.5)).astype(np.int64) * 5
        labels = ids // 5 % 4
        ids[xyz[:, 2] > 4.8] = -1
        scenes.append((xyz, None, labels, ids))
    ignore, min_conf = ((), 0.0) if grid is None else ((0,), 0.26)
    kw = dict(radius=0.2, min_points=3, ignore_classes=ignore, min_confidence=min_conf, votes=1, batch_size=4, seed=2, grid=grid)
    np.random.seed(5)
    got = gpu_model.evaluate_instances(scenes, min_gt_points=50, **kw)
    np.random.seed(5)
    ev = InstanceEvaluator(4, ignore_classes=ignore, min_gt_points=50, device="cpu")
    n_pred = 0
    for xyz, features, labels, ids in scenes:
        res = gpu_model.predict_instances(xyz, features, **kw)
        ev.add(res.instance, res.classes, res.score, ids, labels)
        n_pred += res.count.shape[0]
    same_result(got, ev.result())
    print(f"evaluate_instances grid={grid}: {n_pred} predictions, AP25 {got['AP25']}, mCov {got['mCov']}")
    assert sum(got[f"class {c} n_pred"] for c in range(4)) == n_pred and (n_pred >= 1 or grid is not None)
    assert sum(got[f"class {c} n_gt"] for c in range(4)) == (8 if grid is None else 6)
