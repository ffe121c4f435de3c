"""Keypoints on the MI355X: csrc/keypoints.hip against the numpy twin (utils/keypoints.py) on every case of
tests/keypoints_inputs.py, bit for bit on every array; Model.predict_keypoints on a GPU-placed model against the three steps -
votes, labels twin, peaks twin - run on that model's own voted probabilities; Model.evaluate_keypoints against the evaluator."""
import numpy as np
import pytest
import torch

import keypoints_inputs as ki

pytestmark = pytest.mark.gpu
F32 = np.float32


def _dev():
    return torch.device("cuda", 0)


@pytest.mark.parametrize("name", ki.CASES)
def test_device_equals_the_twin(name):
    from randlanet.utils.keypoints import confidence_peaks
    xyz, lab, sc, r, kw = ki.case(name)
    res = confidence_peaks(xyz, lab, sc, radius=r, device=_dev(), **kw)
    ki.assert_same(res, ki.twin(name), name)


def test_default_device_last_kernel_and_nothing_live():
    from randlanet import _hip
    from randlanet.utils.keypoints import confidence_peaks
    xyz, lab, sc, r, kw = ki.case("uniform_4097")
    res = confidence_peaks(xyz, lab, sc, radius=r, **kw)                # device=None: a GPU is available
    assert res.index.size > 0 and _hip.lib().rl_last_kernel() == b"kp_refine"
    ki.assert_same(res, ki.twin("uniform_4097"))
    # min_points above every support: nothing is live, nothing is refined
    res = confidence_peaks(xyz, lab, sc, radius=r, min_points=5000, device="cuda")
    assert _hip.lib().rl_last_kernel() == b"kp_write"
    for f in ki.FIELDS:
        a = getattr(res, f)
        assert a.dtype == ki.DTYPES[f] and a.shape == ((0, 3) if f == "position" else (0,)), f


def test_many_ignored_classes():
    from randlanet.utils.keypoints import confidence_peaks, confidence_peaks_host
    xyz, lab, sc, r, _ = ki.case("uniform_4097")
    lab = lab.copy()
    lab[::5] = 100 + np.arange(lab[::5].shape[0]) % 40
    ignore = tuple(range(100, 140)) + (0,)
    want = confidence_peaks_host(xyz, lab, sc, radius=r, ignore_classes=ignore, min_points=2)
    ki.assert_same(confidence_peaks(xyz, lab, sc, radius=r, ignore_classes=ignore, min_points=2, device=_dev()), want)
    assert want.index.size > 50 and not np.isin(want.classes, ignore).any()


def test_too_fine_a_grid_is_refused_from_the_device_dims():
    from randlanet.utils.keypoints import confidence_peaks
    xyz, lab, sc = ki.too_fine()
    with pytest.raises(ValueError, match=r"reach 2\^16 = 65536 cells on an axis"):
        confidence_peaks(xyz, lab, sc, radius=1.0, device=_dev())
    res = confidence_peaks(xyz, lab, sc, radius=1.1, device=_dev())
    assert res.index.tolist() == [0, 1, 2] and res.count.tolist() == [1, 1, 1] and np.array_equal(res.position, xyz)


def test_workspace_bytes():
    from randlanet import _hip
    lib = _hip.lib()
    assert lib.rl_keypoints_workspace_bytes(0) == 0 and lib.rl_keypoints_workspace_bytes(2 ** 31 - 1) == 0
    for M in (1, 63, 64, 2047, 2048, 2049, 4097, 10 ** 7, 2 ** 31 - 2):
        n = lib.rl_keypoints_workspace_bytes(M)
        assert n > 52 * M and n % 256 == 0, M


# --------------------------------------------------------------------------------------------------------- Model
@pytest.fixture(scope="module")
def gpu_model():
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    model = Model(RandLANetSettings(n_classes=4, n_points=2048, n_neighbors=8, layer_sizes=[16, 32]), use_gpu=True)
    assert model.device.type == "cuda"
    return model


def _steps(model, xyz, grid, min_points):
    """(keywords, the twins' KeypointResult) of one scene from the model's own voted probabilities; the threshold is their
    median confidence (an untrained network is nowhere sure), so that half of the points take part."""
    from randlanet._scene_path import VoteOptions
    from randlanet.utils import cluster as K
    from randlanet.utils.keypoints import confidence_peaks_host
    np.random.seed(5)
    opt = VoteOptions(votes=1, batch_size=4, smooth=0.95, seed=2, grid=grid)
    prob, _, inverse, V, cloud, *_ = model._scene_path.vote(xyz, None, opt, device_out=True)
    assert prob.is_cuda
    cloud = cloud.cpu().numpy() if torch.is_tensor(cloud) else cloud
    label, conf = K.scene_labels(prob.cpu().numpy())
    kw = dict(radius=0.3, min_score=float(np.median(conf)), min_points=min_points, ignore_classes=())
    want = confidence_peaks_host(cloud[:, :3], label, conf, **kw)
    if grid is not None:
        inv = inverse.cpu().numpy()
        assert 2048 < V < xyz.shape[0] and inv.shape == (xyz.shape[0],)
        first = np.full(V, xyz.shape[0], np.int64)
        np.minimum.at(first, inv, np.arange(xyz.shape[0]))
        assert (inv[first[want.index]] == want.index).all()
        want = want._replace(index=first[want.index])
    else:
        assert inverse is None and V == xyz.shape[0]
    return kw, want


@pytest.mark.parametrize("grid", [None, 0.25])
def test_predict_keypoints_is_the_three_steps_on_its_own_votes(gpu_model, grid):
    rs = np.random.RandomState(11)
    M = 12000
    xyz = rs.uniform(0, 5, (M, 3)).astype(F32)
    kw, want = _steps(gpu_model, xyz, grid, 2)
    np.random.seed(5)
    got = gpu_model.predict_keypoints(xyz, votes=1, batch_size=4, seed=2, grid=grid, **kw)
    ki.assert_same(got, want, f"grid={grid}")
    print(f"predict_keypoints grid={grid}: {got.index.size} keypoints, classes {np.bincount(got.classes, minlength=4).tolist()}")
    assert got.index.size >= 1 and (got.score >= F32(kw["min_score"])).all() and (got.count >= 1).all()
    assert np.array_equal(got.index, np.sort(got.index)) or grid is not None


def test_evaluate_keypoints_is_the_evaluator_on_the_predictions(gpu_model):
    from randlanet.utils.keypoint_metrics import KeypointEvaluator
    rs = np.random.RandomState(12)
    scenes = []
    for k in range(2):
        xyz = rs.uniform(0, 5, (12000, 3)).astype(F32)
        gt = xyz[rs.choice(12000, 40, replace=False)]
        scenes.append((xyz, None, gt) if k == 0 else (xyz, None, gt, rs.randint(1, 4, 40)))
    kw = dict(radius=0.3, min_score=0.0, min_points=2, ignore_classes=(), votes=1, batch_size=4, seed=2)
    np.random.seed(5)
    got = gpu_model.evaluate_keypoints(scenes, distances=(0.15, 0.3), **kw)
    ev = KeypointEvaluator(4, (0.15, 0.3), ignore_classes=())
    np.random.seed(5)
    for sc in scenes:
        res = gpu_model.predict_keypoints(sc[0], **kw)
        assert res.index.size > 10
        ev.add(res.position, res.classes, res.score, sc[2], sc[3] if len(sc) == 4 else None)
    want = ev.result()
    assert list(got) == list(want) and all(got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])) for k in got)
    assert "AP@0.3" in got and "class 3 distance@0.15" in got
