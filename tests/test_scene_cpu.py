"""Model.predict_scene without a GPU: the numpy twin of the scene kernels (utils/scene.py) against brute-force
restatements, the CPU-placed model end to end, and the host-side argument checks of the rl_scene_* entry points."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lexsort_crop(d2: np.ndarray, n: int) -> np.ndarray:
    """The n smallest keys (d2_i, i), by brute force, in ascending index order."""
    return np.sort(np.lexsort((np.arange(d2.shape[0]), d2))[:n])


def _tie_heavy(rs: np.random.RandomState, M: int) -> np.ndarray:
    """Quantised coordinates (many equal distances) with duplicated points."""
    xyz = np.floor(rs.uniform(0, 6, (M, 3))).astype(np.float32) * np.float32(0.5)
    dup = rs.randint(0, M, M // 4)
    xyz[rs.randint(0, M, M // 4)] = xyz[dup]
    return xyz


@pytest.mark.parametrize("kind", ["random", "ties"])
@pytest.mark.parametrize("M", [500, 1000, 5000])
def test_twin_crop_is_the_lexsort_prefix(kind, M):
    from randlanet.utils import scene
    n = 1000
    rs = np.random.RandomState(M + (kind == "ties"))
    xyz = rs.uniform(-3, 3, (M, 3)).astype(np.float32) if kind == "random" else _tie_heavy(rs, M)
    poss = scene.initial_possibility(M, seed=M)
    for _ in range(4):
        c = scene.pick(poss)
        d2 = scene.squared_distances(xyz, c)
        k = min(n, M)
        before = poss.copy()
        idx = scene.crop(xyz, poss, k)
        assert np.array_equal(idx, _lexsort_crop(d2, k))
        assert np.all(np.diff(idx) > 0)
        # possibilities rise by (1 - d2/d2max)^2 on the crop only: the centre by 1, the farthest crop point by 0
        dmax = d2[idx].max()
        assert poss[c] == np.float32(before[c] + 1)
        if dmax > 0:
            assert poss[idx[np.argmax(d2[idx])]] == before[idx[np.argmax(d2[idx])]]
        rest = np.ones(M, bool)
        rest[idx] = False
        assert np.array_equal(poss[rest], before[rest])


def test_twin_distance_expression():
    from randlanet.utils import scene
    rs = np.random.RandomState(0)
    xyz = rs.standard_normal((300, 3)).astype(np.float32)
    d2 = scene.squared_distances(xyz, 7)
    d = xyz[7] - xyz
    ref = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert d2.dtype == np.float32 and np.array_equal(d2.view(np.uint32), ref.view(np.uint32))


def test_pick_breaks_ties_by_lowest_index():
    from randlanet.utils import scene
    p = np.array([3, 1, 2, 1, 1], np.float32)
    assert scene.pick(p) == 1
    p[1] = 5
    assert scene.pick(p) == 3
    assert scene.pick(np.zeros(10, np.float32)) == 0


def test_accumulate_blend_and_counts():
    from randlanet.utils import scene
    rs = np.random.RandomState(1)
    M, C = 50, 3
    prob = np.zeros((M, C), np.float32)
    count = np.zeros(M, np.int32)
    s, oms = scene.blend_factors(0.95)
    assert oms == np.float32(1.0 - 0.95)
    a, b = np.arange(0, 30), np.arange(20, 50)           # overlapping crops
    la, lb = rs.standard_normal((C, 30)).astype(np.float32), rs.standard_normal((C, 30)).astype(np.float32)
    scene.accumulate(prob, count, la, a, oms, s)
    scene.accumulate(prob, count, lb, b, oms, s)
    sa, sb = torch.softmax(torch.from_numpy(la), 0).numpy().T, torch.softmax(torch.from_numpy(lb), 0).numpy().T
    ref = np.zeros((M, C), np.float64)
    ref[a] = 0.05 * sa
    ref[b] = 0.95 * ref[b] + 0.05 * sb
    assert np.allclose(prob, ref, rtol=1e-6, atol=1e-8)
    assert np.array_equal(count, (np.arange(M) < 30).astype(np.int32) + (np.arange(M) >= 20))
    out = scene.normalise(prob)
    assert out.shape == (C, M) and np.abs(out.sum(0) - 1).max() < 1e-6


# ------------------------------------------------------------------------------------------- CPU-placed model
def _model(n_points=2048, n_classes=5, n_features=0, seed=0):
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(seed)
    return Model(RandLANetSettings(n_classes=n_classes, n_points=n_points, n_features=n_features, n_neighbors=8,
                                   layer_sizes=[16, 32]), use_gpu=False)


def _scene(M, seed=0):
    rs = np.random.RandomState(seed)
    return rs.uniform(0, 20, (M, 3)).astype(np.float32)


@pytest.fixture(scope="module")
def cpu_model():
    return _model()


@pytest.mark.parametrize("votes", [1, 2])
def test_predict_scene_cpu_covers_every_point(cpu_model, votes):
    xyz = _scene(20000)
    np.random.seed(11)
    state0 = np.random.get_state()
    out, counts = cpu_model.predict_scene(xyz, votes=votes, batch_size=4, return_counts=True)
    C, M, n, B = cpu_model.settings.n_classes, xyz.shape[0], cpu_model.settings.n_points, 4
    assert out.shape == (C, M) and out.dtype == np.float32
    assert np.abs(out.sum(axis=0) - 1).max() < 1e-5
    assert counts.shape == (M,) and counts.min() >= votes
    # every pass is B crops of n points and one forward, which draws exactly one permutation(n) from the global stream
    assert counts.sum() % (B * n) == 0
    passes = int(counts.sum()) // (B * n)
    ref = np.random.RandomState()
    ref.set_state(state0)
    for _ in range(passes):
        ref.permutation(n)
    after = np.random.get_state()
    assert np.array_equal(ref.get_state()[1], after[1]) and ref.get_state()[2] == after[2]
    # the same seeds give the same result, bit for bit
    np.random.seed(11)
    out2, counts2 = cpu_model.predict_scene(xyz, votes=votes, batch_size=4, return_counts=True)
    assert np.array_equal(out, out2) and np.array_equal(counts, counts2)


def test_predict_scene_cpu_with_features():
    m = _model(n_features=2, n_classes=3)
    rs = np.random.RandomState(2)
    xyz = _scene(6000, seed=2)
    feats = rs.standard_normal((6000, 2)).astype(np.float32)
    np.random.seed(0)
    out, counts = m.predict_scene(xyz, feats, batch_size=2, seed=4, return_counts=True)
    assert out.shape == (3, 6000) and counts.min() >= 1
    assert np.abs(out.sum(axis=0) - 1).max() < 1e-5


def test_predict_scene_small_scene_equals_predict(cpu_model):
    xyz = _scene(1500, seed=3)                  # M <= n_points: every crop is the whole cloud
    np.random.seed(5)
    ref = cpu_model.predict(xyz, prepostprocess=False)
    np.random.seed(5)
    out = cpu_model.predict_scene(xyz)
    assert out.shape == ref.shape
    assert np.abs(out - ref).max() < 1e-6


def test_predict_scene_max_passes_raises(cpu_model):
    xyz = _scene(20000)
    with pytest.raises(RuntimeError, match=r"\d+ of 20000 points were in fewer than 1 crops"):
        cpu_model.predict_scene(xyz, batch_size=1, max_passes=2)


def test_predict_scene_too_small_scene_is_refused(cpu_model):
    n_min = cpu_model.module._min_n_points
    with pytest.raises(AssertionError, match=f"at least {n_min} points"):
        cpu_model.predict_scene(_scene(n_min - 1))


# --------------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def lib():
    from randlanet import _hip
    if not os.path.exists(_hip.library_path()):
        subprocess.check_call(["make", "-C", os.path.join(REPO, "3d_recognizer_amd", "csrc"), "-j4"])
    return _hip.lib()


def test_scene_symbols_are_exported(lib):
    from randlanet import _hip
    raw = ctypes.CDLL(_hip.library_path())
    for name in ("rl_scene_workspace_bytes", "rl_scene_crop", "rl_scene_accumulate", "rl_scene_min_count"):
        assert name in _hip.EXPORTS and hasattr(raw, name)


def test_scene_argument_errors_on_the_host(lib):
    from randlanet import _hip
    M, n = 1000, 100
    need = lib.rl_scene_workspace_bytes(M, n)
    assert need >= 4 * M and lib.rl_scene_workspace_bytes(0, 1) == 0
    fake = 1 << 20              # never dereferenced: every call below is refused before a launch
    assert lib.rl_scene_crop(fake, M, 3, fake, M + 1, fake, 3, fake, fake, need, None) == _hip.ERR_ARGS
    assert b"n=1001" in lib.rl_last_error()
    assert lib.rl_scene_crop(fake, M, 2, fake, n, fake, 2, fake, fake, need, None) == _hip.ERR_ARGS
    assert b"dim=2" in lib.rl_last_error()
    assert lib.rl_scene_crop(fake, M, 3, fake, n, fake, 3, fake, fake, need - 1, None) == _hip.ERR_ARGS
    assert b"workspace" in lib.rl_last_error()
    assert lib.rl_scene_crop(fake, M, 4, fake, n, fake, 3, fake, fake, need, None) == _hip.ERR_ARGS
    assert lib.rl_scene_crop(None, M, 3, fake, n, fake, 3, fake, fake, need, None) == _hip.ERR_ARGS
    assert lib.rl_scene_accumulate(fake, 3, M + 1, fake, 0.05, 0.95, fake, fake, M, None) == _hip.ERR_ARGS
    assert lib.rl_scene_accumulate(None, 3, n, fake, 0.05, 0.95, fake, fake, M, None) == _hip.ERR_ARGS
    assert lib.rl_scene_min_count(fake, 0, fake, fake, None) == _hip.ERR_ARGS
    assert lib.rl_scene_min_count(None, M, fake, fake, None) == _hip.ERR_ARGS
