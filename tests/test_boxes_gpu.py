"""Oriented boxes on the MI355X: csrc/boxes.hip against the numpy twin (utils/boxes.py) on every case of
tests/boxes_inputs.py, bit for bit on every field; the fp64 moments against the twin's; the argument checks of the rl_boxes_*
entries; Model.predict_instances(oriented_boxes=True) and Model.evaluate_instances(boxes=True) on a GPU-placed model against
a CPU-placed copy of it."""
import numpy as np
import pytest
import torch

import boxes_inputs as bi

pytestmark = pytest.mark.gpu
F32 = np.float32


def _dev():
    return torch.device("cuda", 0)


@pytest.mark.parametrize("name", bi.CASES)
def test_device_equals_the_twin(name):
    from randlanet.utils.boxes import instance_boxes
    xyz, ids, n_ids = bi.case(name)
    assert xyz.shape[0] <= 200000
    bi.assert_same(instance_boxes(xyz, ids, n_ids, device=_dev()), bi.twin(name), name)


@pytest.mark.parametrize("name", ["chunk_edges", "long_interleaved", "offset_1e4"])
def test_moments_equal_the_twin(name):
    """The fp64 means and covariances before anything is rounded: the fixed order of the sums itself."""
    from randlanet import _ops as ops
    from randlanet.utils import boxes as B
    pts, ids, I = B.check_inputs(*bi.case(name))
    _, count, mean, cov = B.moments_host(pts, ids, I)
    with torch.cuda.device(_dev()):
        res = ops.instance_boxes(torch.from_numpy(pts).to(_dev()), torch.from_numpy(ids).to(_dev()), I, return_moments=True)
    assert res[7].dtype == res[8].dtype == torch.float64
    assert np.array_equal(res[0].cpu().numpy(), count)
    assert np.array_equal(res[7].cpu().numpy(), mean), name
    assert np.array_equal(res[8].cpu().numpy(), cov), name


def test_id_widths_default_device_and_device_tensors():
    from randlanet import _hip
    from randlanet import _ops as ops
    from randlanet.utils.boxes import instance_boxes
    xyz, ids, _ = bi.case("int32_ids")
    assert ids.dtype == np.int32
    want = bi.twin("int32_ids")
    for other in (np.int64, np.int16):
        bi.assert_same(instance_boxes(xyz, ids.astype(other), 3, device=_dev()), want, str(other))
    unsigned = np.where(ids < 0, 200, ids).astype(np.uint8)              # (no negative ids: 200 stands for "none")
    bi.assert_same(instance_boxes(xyz, unsigned, 201, device=_dev()), instance_boxes(xyz, unsigned, 201, device="cpu"), "uint8")
    got = instance_boxes(xyz, ids)                                        # device=None: a GPU is available
    assert _hip.lib().rl_last_kernel() == b"bx_final"
    bi.assert_same(got, want)
    # device tensors in, device tensors out; without n_ids the one read-back of max(ids) + 1; an id >= n_ids has no box
    with torch.cuda.device(_dev()):
        x_d, i_d = torch.from_numpy(xyz.copy()).to(_dev()), torch.from_numpy(ids.copy()).to(_dev())
        res = ops.instance_boxes(x_d, i_d)
        assert all(t.is_cuda for t in res) and res[0].shape == (3,)
        for t, w in zip(res, want):
            assert np.array_equal(t.cpu().numpy(), w)
        res = ops.instance_boxes(x_d, i_d, 2)
        for t, w in zip(res, want):
            assert np.array_equal(t.cpu().numpy(), w[:2])
        none = ops.instance_boxes(x_d, torch.full_like(i_d, -1))
        assert none[0].shape == (0,) and none[4].shape == (0, 3, 3)


def test_entries_refuse_bad_arguments_without_launching():
    from randlanet import _hip
    with torch.cuda.device(_dev()):
        buf = torch.zeros(1 << 20, dtype=torch.uint8, device=_dev())     # a real, aligned device address
        torch.cuda.synchronize()
        assert buf.data_ptr() % 256 == 0
        bi.abi_refusals(_hip.lib(), buf.data_ptr())
        torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------- Model
@pytest.fixture(scope="module")
def models():
    """A GPU-placed model and a CPU-placed copy whose last layer answers class 1 with certainty whatever it is shown
    (weights 0, bias 200: the softmax is exactly (0, 1, 0, 0) in float32 on both placements), so that the two placements
    label and score every point alike and differ in nothing but where the clustering and the boxes run."""
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    st = dict(n_classes=4, n_points=2048, n_neighbors=8, layer_sizes=[16, 32])
    weights = {k: v.detach().clone() for k, v in Model(RandLANetSettings(**st), use_gpu=False).module.state_dict().items()}
    weights["fc_end.3.conv.weight"].zero_()
    weights["fc_end.3.conv.bias"].copy_(torch.tensor([0.0, 200.0, 0.0, 0.0]))
    gpu = Model(RandLANetSettings(**st), weights={k: v.clone() for k, v in weights.items()}, use_gpu=True)
    cpu = Model(RandLANetSettings(**st), weights=weights, use_gpu=False)
    assert gpu.device.type == "cuda" and cpu.device.type == "cpu"
    return gpu, cpu


def _blob_scene(seed, sizes=(1500, 1200, 900, 1400, 1000)):
    rs = np.random.RandomState(seed)
    xyz, ids = [], []
    for k, n in enumerate(sizes):
        p, _ = bi.blob(rs, n, scale=0.08)
        xyz.append(p - p.mean(axis=0) + np.array([4.0 * (k % 3), 4.0 * (k // 3), 0.5 * k], F32))
        ids.append(np.full(n, 3 * k))
    xyz, ids = np.concatenate(xyz).astype(F32), np.concatenate(ids)
    p = rs.permutation(ids.shape[0])
    return xyz[p], ids[p], (ids[p] // 3 % 2 + 1).astype(np.int64)


KW = dict(radius=0.2, min_points=10, votes=1, batch_size=4, seed=2)


@pytest.mark.parametrize("grid", [None, 0.05])
def test_predict_instances_with_oriented_boxes_equals_the_cpu_placed_model(models, grid):
    gpu, cpu = models
    xyz, _, _ = _blob_scene(3)
    np.random.seed(5)
    got = gpu.predict_instances(xyz, oriented_boxes=True, grid=grid, **KW)
    np.random.seed(5)
    want = cpu.predict_instances(xyz, oriented_boxes=True, grid=grid, **KW)
    np.random.seed(5)
    plain = gpu.predict_instances(xyz, grid=grid, **KW)
    assert type(got).__name__ == type(want).__name__ == "OrientedInstanceResult" and type(plain).__name__ == "InstanceResult"
    assert got.count.shape[0] >= 5 and (got.label == 1).all() and (got.score == 1).all()
    for f, a, b in zip(got._fields, got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b), (grid, f)
    for a, b in zip(plain, got[:8]):
        assert np.array_equal(a, b)
    big = np.argsort(-got.count)[:5]                 # the five blobs: 4 : 2 : 1 boxes, longest axis first
    assert (got.box_extent[big, 0] > got.box_extent[big, 1]).all() and (got.box_extent[big, 1] > got.box_extent[big, 2]).all()


def test_evaluate_instances_with_boxes_on_both_placements(models):
    gpu, cpu = models
    scenes = []
    for seed in (3, 4):
        xyz, ids, labels = _blob_scene(seed)
        scenes.append((xyz, None, labels, ids))
    np.random.seed(5)
    got = gpu.evaluate_instances(scenes, boxes=True, **KW)
    np.random.seed(5)
    want = cpu.evaluate_instances(scenes, boxes=True, **KW)
    np.random.seed(5)
    off = gpu.evaluate_instances(scenes, boxes=False, **KW)
    np.random.seed(5)
    plain = gpu.evaluate_instances(scenes, **KW)
    cols = ("AP", "AP50", "AP25", "precision50", "recall50", "Cov", "WCov", "n_gt", "n_pred")
    parent = ["AP", "AP50", "AP25", "precision50", "recall50", "mCov", "mWCov"] + [f"class {c} {k}" for c in range(4) for k in cols]
    assert list(off) == list(plain) == parent
    box_keys = [k for k in got if k not in parent]
    assert list(got) == parent + box_keys == list(want)
    assert box_keys[:2] == ["box_AP25", "box_AP50"] and "class 1 box_AP50" in box_keys and all("box_" in k for k in box_keys)
    for k in got:
        assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])), k
    for k in parent:
        assert got[k] == off[k] or (np.isnan(got[k]) and np.isnan(off[k])), k
    print({k: got[k] for k in box_keys})
    # every blob is found, as a box of class 1 and score 1: the six class-1 blobs are all matched among the ten predictions
    # (recall reaches 1 at a precision of 6 / 10 or better), the four class-2 ones are missed
    assert got["class 1 box_n_gt"] == 6 and got["class 2 box_n_gt"] == 4 and got["class 1 box_n_pred"] == 10
    assert 0.6 <= got["class 1 box_AP50"] <= got["class 1 box_AP25"] <= 1.0 and got["class 2 box_AP25"] == 0.0
