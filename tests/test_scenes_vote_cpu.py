"""Model.predict_scenes without a GPU: the numpy twin of rl_scenes_vote_crop / rl_scenes_vote_accumulate (utils/scene.py)
against the one-scene twin - every scene's crops are a prefix of the crops predict_scene takes on it alone -, the pass
counts that follow, idle slots, the CPU-placed model end to end, and the host-side argument checks of the new entries."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# above n, at n, one below, not dividing n, one point past a 256-thread tile, one wavefront, a single point
SIZES = [6000, 4096, 4095, 1365, 257, 64, 1]


def _lattice(rs, M):
    """The clouds of tests/test_scene_pad_gpu.py: a coarse lattice (many equal distances), a quarter of the points doubled."""
    ext = max(4.0, round(M ** (1 / 3)))
    x = np.floor(rs.uniform(0, ext, (M, 3))).astype(np.float32) * np.float32(0.25)
    if M >= 4:
        x[rs.randint(0, M, M // 4)] = x[rs.randint(0, M, M // 4)]
    return x


def _run_twin(clouds, n, B, votes, seed=0, pad=True):
    """The passes of predict_scenes by the twin alone (no network).  Returns (crops per scene as lists of LOCAL slot
    rows, passes, idle slots, the slot order of the scenes, final state)."""
    from randlanet.utils import scene
    sizes = [c.shape[0] for c in clouds]
    xyz = np.concatenate(clouds)
    off = scene.scene_offsets(sizes)
    poss = np.concatenate([scene.initial_possibility(M, seed) for M in sizes])
    count = np.zeros(xyz.shape[0], np.int32)
    per = [[] for _ in sizes]
    passes = idle = 0
    order = []
    while True:
        for _ in range(B):
            r = scene.scenes_vote_crop(xyz, off, poss, count, votes, n, pad)
            if r is None:
                idle += 1
                order.append(-1)
                continue
            s, rows, first = r
            assert first == min(n, sizes[s])
            per[s].append(rows - off[s])
            order.append(s)
        passes += 1
        if scene.scenes_low(off, count).min() >= votes:
            break
        assert passes < 100
    return per, passes, idle, order, (poss, count)


def _solo(cloud, n, votes, seed=0, pad=True):
    """The crops predict_scene's twin takes on one scene alone, up to the first one after which every point has `votes`."""
    from randlanet.utils import scene
    M = cloud.shape[0]
    poss = scene.initial_possibility(M, seed)
    count = np.zeros(M, np.int32)
    crops = []
    while count.min() < votes:
        slots = scene.crop(cloud, poss, n, pad=pad)
        count[slots[:min(n, M)]] += 1
        crops.append(slots)
    return crops, poss, count


@pytest.fixture(scope="module")
def lattice_clouds():
    rs = np.random.RandomState(7)
    return [_lattice(rs, M) for M in SIZES]


@pytest.mark.parametrize("votes,want_passes", [(1, 3), (2, 5)])
def test_every_scenes_crops_are_a_prefix_of_its_solo_sequence(lattice_clouds, votes, want_passes):
    n, B = 4096, 4
    per, passes, idle, order, (poss, count) = _run_twin(lattice_clouds, n, B, votes)
    total = 0
    at = 0
    for s, cloud in enumerate(lattice_clouds):
        solo, solo_poss, solo_count = _solo(cloud, n, votes)
        assert len(per[s]) == len(solo), f"scene {s}: {len(per[s])} crops together, {len(solo)} alone"
        for k, (a, b) in enumerate(zip(per[s], solo)):
            assert np.array_equal(a, b), f"scene {s}, crop {k}"
        M = cloud.shape[0]
        assert np.array_equal(poss[at:at + M].view(np.uint32), solo_poss.view(np.uint32))
        assert np.array_equal(count[at:at + M], solo_count)
        at += M
        total += len(solo)
    # idle slots can only follow the last crop, so the passes are the crops of the scene-by-scene loop packed B per pass
    assert passes == -(-total // B) == want_passes
    assert idle == passes * B - total
    assert all(s == -1 for s in order[total:]) and all(s >= 0 for s in order[:total])


def test_five_small_scenes_take_one_slot_each():
    rs = np.random.RandomState(7)
    sizes = [900, 700, 1500, 300, 1200]
    clouds = [rs.uniform(0, 10, (M, 3)).astype(np.float32) for M in sizes]
    per, passes, idle, order, (_, count) = _run_twin(clouds, 2048, 4, 1)
    assert [len(p) for p in per] == [1] * 5
    assert passes == 2 and idle == 3
    assert sorted(order[:5]) == [0, 1, 2, 3, 4] and order[5:] == [-1] * 3
    assert np.all(count == 1)
    for s, M in enumerate(sizes):
        assert np.array_equal(per[s][0], np.resize(np.arange(M), 2048))


def test_an_idle_slot_changes_nothing():
    from randlanet.utils import scene
    rs = np.random.RandomState(1)
    sizes = [300, 500]
    xyz = rs.uniform(0, 4, (800, 3)).astype(np.float32)
    off = scene.scene_offsets(sizes)
    poss = np.concatenate([scene.initial_possibility(M, 0) for M in sizes])
    count = np.zeros(800, np.int32)
    assert scene.scenes_vote_crop(xyz, off, poss, count, 1, 256, True)[0] in (0, 1)
    count[:] = 1                                        # every scene covered
    p0, c0 = poss.copy(), count.copy()
    assert scene.scenes_vote_crop(xyz, off, poss, count, 1, 256, True) is None
    assert np.array_equal(p0.view(np.uint32), poss.view(np.uint32)) and np.array_equal(c0, count)
    prob = rs.uniform(0, 1, (800, 3)).astype(np.float32)
    before = prob.copy()
    scene.scenes_vote_accumulate(prob, np.full((3, 256), 1e30, np.float32), np.arange(256), np.float32(0.05),
                                 np.float32(0.95), 0)
    assert np.array_equal(before, prob)
    # a closed scene is skipped although it holds the least possibility
    count[:] = 0
    count[:300] = 1
    poss[:300] = 0
    s, rows, first = scene.scenes_vote_crop(xyz, off, poss, count, 1, 256, True)
    assert s == 1 and first == 256 and rows.min() >= 300


def test_vote_accumulate_is_accumulate_first_without_the_count():
    from randlanet.utils import scene
    rs = np.random.RandomState(2)
    T, C, n, first = 500, 5, 256, 100
    s, oms = scene.blend_factors(0.95)
    idx = 200 + np.resize(np.arange(first), n)
    lg = (3 * rs.standard_normal((C, n))).astype(np.float32)
    lg[0, first:] = 1e30
    a = rs.uniform(0, 1, (T, C)).astype(np.float32)
    b = a.copy()
    cnt = np.zeros(T, np.int32)
    scene.accumulate(a, cnt, lg, idx, oms, s, first=first)
    scene.scenes_vote_accumulate(b, lg, idx, oms, s, first)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------- CPU-placed model
def _model(n_points=2048, n_classes=5, n_features=0, seed=0):
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(seed)
    return Model(RandLANetSettings(n_classes=n_classes, n_points=n_points, n_features=n_features, n_neighbors=8,
                                   layer_sizes=[16, 32]), use_gpu=False)


@pytest.fixture(scope="module")
def cpu_model():
    return _model()


def _scenes(sizes, seed=0, extent=10.0):
    rs = np.random.RandomState(seed)
    return [(rs.uniform(0, extent, (M, 3)).astype(np.float32), None) for M in sizes]


@pytest.mark.parametrize("votes", [1, 2])
def test_predict_scenes_cpu_model(cpu_model, votes):
    sizes, n, B = [3000, 700, 2500, 40], 2048, 3
    scenes = _scenes(sizes, seed=3)
    np.random.seed(11)
    state0 = np.random.get_state()
    out, counts, info = cpu_model.predict_scenes(scenes, votes=votes, batch_size=B, seed=2, return_counts=True,
                                                 return_info=True, pad_small_scenes=True)
    after = np.random.get_state()
    assert len(out) == len(counts) == len(sizes)
    for M, o, c in zip(sizes, out, counts):
        assert o.shape == (5, M) and o.dtype == np.float32
        assert np.abs(o.sum(axis=0) - 1).max() < 1e-5
        assert c.shape == (M,) and c.min() >= votes
    per, passes, _, _, (_, count) = _run_twin([x for x, _ in scenes], n, B, votes, seed=2)
    assert info["passes"] == passes
    assert np.array_equal(info["crops"], [len(p) for p in per])
    assert np.array_equal(np.concatenate(counts), count)
    # one forward per pass: the global numpy stream advances by exactly `passes` permutations of n
    ref = np.random.RandomState()
    ref.set_state(state0)
    for _ in range(passes):
        ref.permutation(n)
    assert np.array_equal(ref.get_state()[1], after[1]) and ref.get_state()[2] == after[2]
    # the plain return, and the same seeds give the same bits
    np.random.seed(11)
    again = cpu_model.predict_scenes(scenes, votes=votes, batch_size=B, seed=2, pad_small_scenes=True)
    assert isinstance(again, list) and all(np.array_equal(a, b) for a, b in zip(again, out))


def test_predict_scenes_groups_by_resident_points(cpu_model):
    """Two groups ([3000], [700, 2500]): each group's scenes compete with each other only."""
    scenes = _scenes([3000, 700, 2500], seed=3)
    np.random.seed(1)
    _, info = cpu_model.predict_scenes(scenes, batch_size=2, pad_small_scenes=True, max_resident_points=3200,
                                       return_info=True)
    a = _run_twin([scenes[0][0]], 2048, 2, 1)
    b = _run_twin([scenes[1][0], scenes[2][0]], 2048, 2, 1)
    assert info["passes"] == a[1] + b[1]
    assert np.array_equal(info["crops"], [len(p) for p in a[0] + b[0]])


def test_predict_scenes_small_scene_needs_pad_small_scenes(cpu_model):
    scenes = _scenes([3000, 700], seed=3)
    with pytest.raises(ValueError, match="scene 1 has 700 points, fewer than the crop size n=2048"):
        cpu_model.predict_scenes(scenes)


def test_predict_scenes_max_passes_raises(cpu_model):
    scenes = _scenes([700, 20000, 900], seed=3, extent=20.0)
    with pytest.raises(RuntimeError, match=r"scenes \[[\d, ]+\] have points in fewer than 1 crops after max_passes=2 passes"):
        cpu_model.predict_scenes(scenes, batch_size=2, max_passes=2, pad_small_scenes=True)


def test_predict_scenes_grid_carries_every_cells_column_to_its_raw_points(cpu_model):
    from randlanet.utils import grid as grid_utils
    scenes = _scenes([9000, 1200], seed=5, extent=4.0)
    cell = 0.25
    subs = [grid_utils.grid_subsample_host(x, None, cell=cell) for x, _ in scenes]
    assert subs[0].xyz.shape[0] >= 2048 > subs[1].xyz.shape[0]
    np.random.seed(3)
    out, counts = cpu_model.predict_scenes(scenes, batch_size=2, grid=cell, pad_small_scenes=True, return_counts=True)
    np.random.seed(3)
    ref, ref_counts = cpu_model.predict_scenes([(s.xyz, None) for s in subs], batch_size=2, pad_small_scenes=True,
                                               return_counts=True)
    for (x, _), s, o, c, r, rc in zip(scenes, subs, out, counts, ref, ref_counts):
        assert o.shape == (5, x.shape[0]) and c.shape == (x.shape[0],)
        assert np.array_equal(o, r[:, s.inverse]) and np.array_equal(c, rc[s.inverse])


def test_evaluate_scenes_together_cpu_model(cpu_model):
    from randlanet.utils import grid as grid_utils
    rs = np.random.RandomState(6)
    scenes = [(x, None, rs.randint(-1, 5, x.shape[0])) for x, _ in _scenes([3000, 700], seed=4)]
    np.random.seed(2)
    out, conf = cpu_model.evaluate_scenes(scenes, batch_size=2, pad_small_scenes=True, together=True,
                                          return_confusion=True)
    np.random.seed(2)
    probs = cpu_model.predict_scenes(scenes, batch_size=2, pad_small_scenes=True)
    want = sum(grid_utils.confusion(np.ascontiguousarray(p.T), l, 5) for p, (_, _, l) in zip(probs, scenes))
    assert conf.sum() == sum(int((l >= 0).sum()) for _, _, l in scenes)
    assert np.array_equal(conf, want) and 0.0 <= out["OA"] <= 1.0


# --------------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def lib():
    from randlanet import _hip
    if not os.path.exists(_hip.library_path()):
        subprocess.check_call(["make", "-C", os.path.join(REPO, "3d_recognizer_amd", "csrc"), "-j4"])
    return _hip.lib()


def test_vote_symbols_are_exported(lib):
    from randlanet import _hip
    raw = ctypes.CDLL(_hip.library_path())
    for name in ("rl_scenes_vote_crop", "rl_scenes_vote_accumulate"):
        assert name in _hip.EXPORTS and hasattr(raw, name)
    assert lib.rl_version() == _hip.ABI_VERSION


def test_vote_argument_errors_on_the_host(lib):
    from randlanet import _hip
    S, Mmax, n, B, dim = 3, 1000, 100, 4, 5
    need = lib.rl_scenes_workspace_bytes(S, Mmax, n)
    fake = 1 << 20              # never dereferenced: every call below is refused before a launch

    def crop(cloud=fake, dim=dim, S=S, Mmax=Mmax, count=fake, votes=1, n=n, B=B, pad=0, slot=n * dim, row=dim,
             first=fake, ws=fake, ws_bytes=need):
        return lib.rl_scenes_vote_crop(cloud, dim, S, Mmax, fake, count, fake, votes, n, B, pad, fake, slot, row, fake,
                                       fake, first, fake, ws, ws_bytes, None)

    assert crop(S=0) == _hip.ERR_ARGS and b"S=0" in lib.rl_last_error()
    assert crop(B=0) == _hip.ERR_ARGS
    assert crop(votes=0) == _hip.ERR_ARGS and b"votes=0" in lib.rl_last_error()
    assert crop(dim=2, row=2, slot=2 * n) == _hip.ERR_ARGS and b"dim=2" in lib.rl_last_error()
    assert crop(n=Mmax + 1, slot=(Mmax + 1) * dim) == _hip.ERR_ARGS and b"n=1001" in lib.rl_last_error()
    assert crop(n=0) == _hip.ERR_ARGS
    assert crop(row=dim - 1) == _hip.ERR_ARGS and b"row_stride" in lib.rl_last_error()
    assert crop(slot=n * dim - 1) == _hip.ERR_ARGS and b"slot_stride" in lib.rl_last_error()
    assert crop(ws_bytes=need - 1) == _hip.ERR_ARGS and b"workspace" in lib.rl_last_error()
    assert crop(ws=fake + 8) == _hip.ERR_ARGS and b"aligned" in lib.rl_last_error()
    assert crop(cloud=None) == _hip.ERR_ARGS and b"null" in lib.rl_last_error()
    assert crop(count=None) == _hip.ERR_ARGS
    assert crop(first=None) == _hip.ERR_ARGS

    def acc(logits=fake, C=13, n=n, ld=n, slot=13 * n, B=B, first=fake, T=1000):
        return lib.rl_scenes_vote_accumulate(logits, C, n, ld, slot, B, fake, first, 0.05, 0.95, fake, T, None)

    assert acc(C=0) == _hip.ERR_ARGS and b"C=0" in lib.rl_last_error()
    assert acc(ld=n - 1) == _hip.ERR_ARGS
    assert acc(T=0) == _hip.ERR_ARGS
    assert acc(B=0) == _hip.ERR_ARGS
    assert acc(slot=12 * n + n - 1) == _hip.ERR_ARGS and b"overlap" in lib.rl_last_error()
    assert acc(logits=None) == _hip.ERR_ARGS and b"null" in lib.rl_last_error()
    assert acc(first=None) == _hip.ERR_ARGS
