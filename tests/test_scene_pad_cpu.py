"""Padded crops (pad_small_scenes) without a GPU: the numpy twin (utils/scene.py crop / scenes_crop with pad=True) against
the unpadded twin where the scene is large enough and against a brute-force restatement where it is not, check_scenes, and
Model.predict_scene(pad_small_scenes=True) on a CPU-placed model."""
import numpy as np
import pytest
import torch

_F32 = np.float32


def _lattice(rs: np.random.RandomState, M: int) -> np.ndarray:
    """Quantised coordinates (many equal distances) with duplicated points."""
    xyz = np.floor(rs.uniform(0, 6, (M, 3))).astype(_F32) * _F32(0.5)
    if M >= 4:
        xyz[rs.randint(0, M, M // 4)] = xyz[rs.randint(0, M, M // 4)]
    return xyz


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------- 1. twin, M >= n
@pytest.mark.parametrize("M,n", [(1000, 1000), (1001, 1000), (5000, 300)])
def test_padded_twin_equals_the_unpadded_twin_on_large_scenes(M, n):
    from randlanet.utils import scene
    rs = np.random.RandomState(M)
    xyz = _lattice(rs, M)
    pa = scene.initial_possibility(M, seed=1)
    pb = pa.copy()
    for k in range(5):
        a, b = scene.crop(xyz, pa, n), scene.crop(xyz, pb, n, pad=True)
        assert np.array_equal(a, b), f"crop {k}"
        assert np.array_equal(_bits(pa), _bits(pb)), f"crop {k}"
    # several scenes, each of n points or more
    sizes = [M, n, 2 * n + 7]
    xyz = np.concatenate([_lattice(rs, m) for m in sizes])
    off = scene.scene_offsets(sizes)
    pa = scene.initial_possibility(xyz.shape[0], seed=2)
    pb = pa.copy()
    for k in range(8):
        nz = rs.normal(0, 0.2, 3).astype(_F32) if k % 2 else None
        (sa, a), (sb, b) = scene.scenes_crop(xyz, off, pa, n, nz), scene.scenes_crop(xyz, off, pb, n, nz, pad=True)
        assert sa == sb and np.array_equal(a, b), f"crop {k}"
        assert np.array_equal(_bits(pa), _bits(pb)), f"crop {k}"


# ------------------------------------------------------------------------------------------------- 2. twin, M < n
def _brute_padded(xyz, centre, before, n):
    """The padded crop of a scene of M < n points, restated: (the n slots, the possibilities afterwards)."""
    M = xyz.shape[0]
    d = centre.astype(_F32) - xyz
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    T = d2.max()
    after = before.copy()
    for i in range(M):
        t = _F32(1) - (d2[i] / T if T != 0 else _F32(0))
        after[i] = before[i] + t * t
    return np.resize(np.arange(M), n), after


@pytest.mark.parametrize("M", [999, 700, 333, 64, 3, 1])
def test_padded_twin_on_a_small_scene(M):
    from randlanet.utils import scene
    n = 1000
    rs = np.random.RandomState(M)
    xyz = _lattice(rs, M)
    poss = scene.initial_possibility(M, seed=M)
    for k in range(3):
        c = scene.pick(poss)
        want_idx, want_poss = _brute_padded(xyz, xyz[c], poss, n)
        idx = scene.crop(xyz, poss, n, pad=True)
        assert idx.shape == (n,) and np.array_equal(idx, want_idx), f"crop {k}"
        occ = np.bincount(idx, minlength=M)
        assert occ.min() >= n // M and occ.max() <= -(-n // M) and occ.sum() == n
        assert np.array_equal(_bits(poss), _bits(want_poss)), f"crop {k}"


def test_padded_twin_small_scene_among_several():
    from randlanet.utils import scene
    n = 1000
    rs = np.random.RandomState(5)
    sizes = [1500, 333, 1000, 1]
    xyz = np.concatenate([_lattice(rs, m) for m in sizes])
    off = scene.scene_offsets(sizes)
    poss = scene.initial_possibility(xyz.shape[0], seed=3)
    seen = set()
    for k in range(12):
        nz = rs.normal(0, 0.2, 3).astype(_F32) if k % 2 else None
        g, s = scene.scenes_pick(poss, off)
        b, e = int(off[s]), int(off[s + 1])
        before = poss.copy()
        centre = xyz[g] if nz is None else xyz[g] + nz
        got_s, idx = scene.scenes_crop(xyz, off, poss, n, nz, pad=True)
        assert got_s == s and idx.shape == (n,)
        if e - b < n:
            want_idx, want = _brute_padded(xyz[b:e], centre, before[b:e], n)
            assert np.array_equal(idx, want_idx + b)
            assert np.array_equal(_bits(poss[b:e]), _bits(want))
        else:
            assert np.all(np.diff(idx) > 0) and idx[0] >= b and idx[-1] < e
        rest = np.ones(poss.shape[0], bool)
        rest[b:e] = False
        assert np.array_equal(_bits(poss[rest]), _bits(before[rest]))
        seen.add(s)
    assert seen == {0, 1, 2, 3}


def test_padded_twin_single_point_and_coincident_scene_add_exactly_one():
    from randlanet.utils import scene
    one = np.array([[1.5, -2.0, 0.25]], _F32)
    poss = np.array([0.125], _F32)
    assert np.array_equal(scene.crop(one, poss, 7, pad=True), np.zeros(7, np.int64))
    assert poss[0] == _F32(1.125)
    same = np.repeat(one, 5, axis=0)                    # T == 0
    poss = np.array([0.5, 0.25, 0.75, 0.25, 1.0], _F32)
    before = poss.copy()
    assert np.array_equal(scene.crop(same, poss, 12, pad=True), np.resize(np.arange(5), 12))
    assert np.array_equal(poss, before + _F32(1))
    # with centre noise the coincident points are all at the same d2 == T != 0: t = 1 - 1 = 0, nothing is added
    poss = before.copy()
    scene.scenes_crop(same, scene.scene_offsets([5]), poss, 12, np.array([0.5, 0, 0], _F32), pad=True)
    assert np.array_equal(poss, before)


def test_accumulate_first_blends_the_leading_slots_only():
    from randlanet.utils import scene
    rs = np.random.RandomState(1)
    M, C, n = 30, 4, 100
    s, oms = scene.blend_factors(0.95)
    idx = np.resize(np.arange(M), n)
    logits = rs.standard_normal((C, n)).astype(_F32)
    prob, count = np.zeros((M, C), _F32), np.zeros(M, np.int32)
    ref, rcount = prob.copy(), count.copy()
    old, ocount = prob.copy(), count.copy()
    scene.accumulate(prob, count, logits, idx, oms, s, first=M)
    scene.accumulate(ref, rcount, np.ascontiguousarray(logits[:, :M]), idx[:M], oms, s, first=M)
    assert np.array_equal(_bits(prob), _bits(ref)) and np.array_equal(count, np.ones(M, np.int32))
    # rl_scene_accumulate's twin on the leading slots: another exp (np.exp), the 1e-6 tests/test_scene_gpu.py holds the
    # kernel's expf to against it
    scene.accumulate(old, ocount, np.ascontiguousarray(logits[:, :M]), idx[:M], oms, s)
    assert np.all(np.abs(prob - old) <= 1e-6 * np.abs(old) + 1e-12) and np.array_equal(count, ocount)


def test_exp_fixed_is_exp():
    """The fixed float32 expression of rl_scene_accumulate_first's softmax against float64 exp.  Bound: Cephes documents
    1.7e-7 relative for this polynomial and reduction; 2 float32 ulp (2^-22 = 2.4e-7) on top of the correctly rounded
    value allows for that."""
    from randlanet.utils import scene
    rs = np.random.RandomState(2)
    x = np.concatenate([-rs.uniform(0, 87, 200000), -rs.uniform(0, 1, 100000),
                        [0.0, -87.0, -0.5 * np.log(2), -1e-8, -86.99999]]).astype(_F32)
    got = scene.exp_fixed(x)
    want = np.exp(x.astype(np.float64))
    assert got.dtype == _F32 and got.shape == x.shape
    rel = float((np.abs(got - want) / want).max())
    print(f"exp_fixed: largest relative error {rel:.3e}")
    assert rel <= 2.0 ** -22
    assert got[x == 0].tolist() == [1.0]
    with np.errstate(invalid="ignore"):
        edge = scene.exp_fixed(np.array([-87.00001, -100.0, -np.inf, np.nan], _F32))
    assert np.array_equal(_bits(edge), np.zeros(4, np.uint32))
    # the softmax: the largest class is exp(0) = 1 exactly, columns sum to 1 within the C roundings of the sum
    lg = (3 * rs.standard_normal((13, 500))).astype(_F32)
    sm = scene.softmax_fixed(lg)
    assert sm.dtype == _F32 and np.all(np.abs(sm.sum(axis=0, dtype=np.float64) - 1) <= 13 * 2.0 ** -24)
    assert np.array_equal(sm.argmax(axis=0), lg.argmax(axis=0))


# ------------------------------------------------------------------------------------------------- 3. check_scenes
def _sample(M, F=2):
    return np.zeros((M, 3), _F32), np.zeros((M, F), _F32), np.zeros(M, np.int64)


def test_check_scenes_accepts_small_scenes_only_with_the_keyword():
    from randlanet.utils.scene_loader import check_scenes
    scenes = [_sample(3000), _sample(700), _sample(1)]
    with pytest.raises(ValueError, match=r"scene 1 has 700 points, fewer than the crop size n=2048"):
        check_scenes(scenes, 2048)
    with pytest.raises(ValueError, match=r"scene 1 has 700 points, fewer than the crop size n=2048"):
        check_scenes(scenes, 2048, pad_small_scenes=False)
    assert check_scenes(scenes, 2048, pad_small_scenes=True) == 2
    empty = [_sample(3000), _sample(0)]
    with pytest.raises(ValueError, match=r"scene 1 has 0 points"):
        check_scenes(empty, 2048)
    with pytest.raises(ValueError, match=r"scene 1 has 0 points"):
        check_scenes(empty, 2048, pad_small_scenes=True)


# ------------------------------------------------------------------------------------------------- 4. CPU-placed model
@pytest.fixture(scope="module")
def cpu_model():
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    return Model(RandLANetSettings(n_classes=5, n_points=2048, n_neighbors=8, layer_sizes=[8, 16, 32, 32]), use_gpu=False)


@pytest.mark.parametrize("votes", [1, 2])
def test_predict_scene_padded_tiny_scene(cpu_model, votes):
    M = 500
    assert M < cpu_model.module._min_n_points
    xyz = np.random.RandomState(1).uniform(0, 5, (M, 3)).astype(_F32)
    with pytest.raises(AssertionError, match="at least"):
        cpu_model.predict_scene(xyz)
    np.random.seed(3)
    state0 = np.random.get_state()
    out, counts = cpu_model.predict_scene(xyz, votes=votes, batch_size=2, return_counts=True, pad_small_scenes=True)
    assert out.shape == (5, M) and out.dtype == _F32
    assert np.abs(out.sum(axis=0) - 1).max() < 1e-5
    # every crop is the whole scene and votes each point once: one pass of two crops covers votes <= 2
    assert counts.shape == (M,) and counts.min() >= votes and np.all(counts == 2)
    ref = np.random.RandomState()
    ref.set_state(state0)
    ref.permutation(2048)                   # the one forward, at n_points
    assert np.array_equal(ref.get_state()[1], np.random.get_state()[1])


def test_predict_scene_padded_is_a_no_op_on_a_large_scene(cpu_model):
    xyz = np.random.RandomState(2).uniform(0, 10, (5000, 3)).astype(_F32)
    np.random.seed(4)
    a, ca = cpu_model.predict_scene(xyz, batch_size=2, return_counts=True)
    np.random.seed(4)
    b, cb = cpu_model.predict_scene(xyz, batch_size=2, return_counts=True, pad_small_scenes=True)
    assert np.array_equal(a, b) and np.array_equal(ca, cb)
    exact = np.random.RandomState(2).uniform(0, 10, (2048, 3)).astype(_F32)      # M == n_points
    np.random.seed(4)
    a = cpu_model.predict_scene(exact)
    np.random.seed(4)
    b = cpu_model.predict_scene(exact, pad_small_scenes=True)
    assert np.array_equal(a, b)


def test_evaluate_scenes_padded_counts_every_raw_point_once(cpu_model):
    rs = np.random.RandomState(6)
    xyz = rs.uniform(0, 5, (300, 3)).astype(_F32)
    labels = rs.randint(-1, 5, 300)                     # -1: unlabelled
    np.random.seed(0)
    _, conf = cpu_model.evaluate_scenes([(xyz, None, labels)], batch_size=1, return_confusion=True, pad_small_scenes=True)
    assert conf.sum() == int((labels >= 0).sum())


# --------------------------------------------------------------------------------------------------- C ABI
def test_padded_entries_check_their_arguments_on_the_host():
    from randlanet import _hip
    lib = _hip.lib()
    M, n = 1000, 4096
    need = lib.rl_scene_workspace_bytes(M, n)
    assert need == lib.rl_scene_workspace_bytes(M, 1)               # the workspace does not depend on n
    fake = 1 << 20              # never dereferenced: every call below is refused before a launch
    assert lib.rl_scene_crop(fake, M, 3, fake, n, fake, 3, fake, fake, need, None) == _hip.ERR_ARGS
    assert b"rl_scene_crop: crop of n=4096 points out of M=1000" in lib.rl_last_error()
    assert lib.rl_scene_crop_padded(fake, M, 3, fake, 0, fake, 3, fake, fake, need, None) == _hip.ERR_ARGS
    assert b"rl_scene_crop_padded: crop of n=0" in lib.rl_last_error()
    assert lib.rl_scene_crop_padded(fake, 0, 3, fake, n, fake, 3, fake, fake, need, None) == _hip.ERR_ARGS
    assert lib.rl_scene_crop_padded(fake, M, 3, fake, n, fake, 3, fake, fake, need - 1, None) == _hip.ERR_ARGS
    assert b"workspace" in lib.rl_last_error()
    assert lib.rl_scene_crop_padded(fake, M, 3, fake, n, fake, 3, None, fake, need, None) == _hip.ERR_ARGS
    # first <= n <= ld, first <= M
    for C, nn, ld, first in ((3, n, n, M + 1), (3, n, n - 1, M), (3, 10, n, 11), (0, n, n, M), (3, n, n, 0)):
        assert lib.rl_scene_accumulate_first(fake, C, nn, fake, 0.05, 0.95, fake, fake, M, ld, first, None) == _hip.ERR_ARGS
        assert b"rl_scene_accumulate_first: bad sizes" in lib.rl_last_error()
    assert lib.rl_scene_accumulate_first(None, 3, n, fake, 0.05, 0.95, fake, fake, M, n, M, None) == _hip.ERR_ARGS
    S, Mmax = 3, 2500
    need = lib.rl_scenes_workspace_bytes(S, Mmax, n)
    assert need == lib.rl_scenes_workspace_bytes(S, Mmax, 1)
    assert lib.rl_scenes_crop(fake, 3, S, Mmax, fake, n, 2, None, fake, fake, fake, need, None) == _hip.ERR_ARGS
    assert b"rl_scenes_crop: crop of n=4096 points, largest scene 2500" in lib.rl_last_error()
    assert lib.rl_scenes_crop_padded(fake, 3, S, Mmax, fake, 0, 2, None, fake, fake, fake, need, None) == _hip.ERR_ARGS
    assert lib.rl_scenes_crop_padded(fake, 2, S, Mmax, fake, n, 2, None, fake, fake, fake, need, None) == _hip.ERR_ARGS
    assert b"rl_scenes_crop_padded: stride=2" in lib.rl_last_error()
    assert lib.rl_scenes_crop_padded(fake, 3, S, Mmax, fake, n, 2, None, fake, fake, fake, need - 1, None) == _hip.ERR_ARGS
    assert lib.rl_scenes_crop_padded(fake, 3, S, Mmax, fake, n, 2, None, None, fake, fake, need, None) == _hip.ERR_ARGS
