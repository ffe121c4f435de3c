"""Voted crops over many scenes on the MI355X: rl_scenes_vote_crop and rl_scenes_vote_accumulate against their numpy twins
(utils/scene.py) bit for bit, against rl_scenes_crop_padded where no scene closes, and Model.predict_scenes /
evaluate_scenes(together=True) against a CPU-placed model with the same weights."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 4096                    # the crop size of the kernel tests
# above n (six select workgroups: the atomicMin on low crosses workgroups), at n, one below, not dividing n, one point past a
# 256-thread tile, one wavefront, a single point
SIZES = [6000, 4096, 4095, 1365, 257, 64, 1]


def _dev():
    return torch.device("cuda", 0)


def _lattice(rs, M):
    """Coarse lattice (many equal distances) with a quarter of the points duplicated, as tests/test_scene_pad_gpu.py."""
    ext = max(4.0, round(M ** (1 / 3)))
    x = np.floor(rs.uniform(0, ext, (M, 3))).astype(np.float32) * np.float32(0.25)
    if M >= 4:
        x[rs.randint(0, M, M // 4)] = x[rs.randint(0, M, M // 4)]
    return x


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("F,extra", [(0, 0), (2, 2)])
@pytest.mark.parametrize("votes", [1, 2])
def test_scenes_vote_crop_bitwise_twin(votes, F, extra):
    from randlanet import _ops as ops
    from randlanet.utils import scene
    rs = np.random.RandomState(7)
    sizes, n, B = SIZES, N, 4
    cloud = np.concatenate([_lattice(rs, M) for M in sizes])
    T, dim = cloud.shape[0], 3 + F
    if F:
        cloud = np.ascontiguousarray(np.concatenate([cloud, rs.standard_normal((T, F)).astype(np.float32)], axis=1))
    off = scene.scene_offsets(sizes)
    poss = np.concatenate([scene.initial_possibility(M, 0) for M in sizes])
    count = np.zeros(T, np.int32)
    dev = _dev()
    S, Mmax = len(sizes), max(sizes)
    passes = idle = 0
    with torch.cuda.device(dev):
        cloud_d = torch.from_numpy(cloud).to(dev)
        poss_d = torch.from_numpy(poss).to(dev)
        count_d = torch.zeros(T, dtype=torch.int32, device=dev)
        low_d = torch.zeros(S, dtype=torch.int32, device=dev)
        ws = ops.scenes_workspace(dev, S, Mmax, n)
        ops.scenes_init(torch.from_numpy(off).to(dev), poss_d, ws, Mmax)
        sc = torch.empty(B, dtype=torch.int64, device=dev)
        first = torch.empty(B, dtype=torch.int32, device=dev)
        open_d = torch.full((1,), -5, dtype=torch.int32, device=dev)
        done = False
        while True:                         # the twin's passes, and one more in which every slot is idle
            want = [scene.scenes_vote_crop(cloud, off, poss, count, votes, n, True) for _ in range(B)]
            rows = torch.full((B, n, dim + extra), -7.0, dtype=torch.float32, device=dev)
            idx = torch.full((B, n), -1, dtype=torch.int64, device=dev)
            sc.fill_(-9)
            first.fill_(-9)
            ops.scenes_vote_crop(cloud_d, poss_d, count_d, low_d, votes, n, rows, idx, sc, first, open_d, ws, S, Mmax, pad=True)
            assert sc.cpu().tolist() == [-1 if w is None else w[0] for w in want], f"pass {passes}: scenes differ"
            assert first.cpu().tolist() == [0 if w is None else w[2] for w in want], f"pass {passes}: first differs"
            got_i, got_r = idx.cpu().numpy(), rows.cpu().numpy()
            for b, w in enumerate(want):
                if w is None:               # idle: the sentinels are still there
                    assert np.all(got_i[b] == -1) and np.all(got_r[b] == -7.0), f"pass {passes}, slot {b}: idle slot written"
                    idle += 1
                    continue
                assert np.array_equal(got_i[b], w[1]), f"pass {passes}, crop {b}: indices differ"
                assert np.array_equal(_bits(got_r[b][:, :dim]), _bits(cloud[w[1]])), f"pass {passes}, crop {b}: rows differ"
                assert np.all(got_r[b][:, dim:] == -7.0)
            assert np.array_equal(_bits(poss_d.cpu().numpy()), _bits(poss)), f"pass {passes}: possibilities differ"
            assert np.array_equal(count_d.cpu().numpy(), count), f"pass {passes}: counts differ"
            low = scene.scenes_low(off, count)
            assert np.array_equal(low_d.cpu().numpy(), low), f"pass {passes}: low differs"
            assert int(open_d.item()) == int((low < votes).sum()), f"pass {passes}: open scenes differ"
            if done:
                assert all(w is None for w in want)
                break
            passes += 1
            done = int(low.min()) >= votes
    assert passes == {1: 3, 2: 5}[votes]        # (tests/test_scenes_vote_cpu.py derives these from the solo sequences)
    assert idle == {1: 2, 2: 1}[votes] + B


def test_scenes_vote_crop_equals_scenes_crop_padded_while_no_scene_closes():
    from randlanet import _ops as ops
    from randlanet.utils import scene
    rs = np.random.RandomState(11)
    sizes, n, B = [6000, 300, 4097, 1000], N, 4
    xyz = np.concatenate([_lattice(rs, M) for M in sizes])
    T = xyz.shape[0]
    off = scene.scene_offsets(sizes)
    poss = scene.initial_possibility(T, seed=4)
    dev = _dev()
    S, Mmax = len(sizes), max(sizes)
    with torch.cuda.device(dev):
        xyz_d = torch.from_numpy(xyz).to(dev)
        off_d = torch.from_numpy(off).to(dev)
        pa = torch.from_numpy(poss).to(dev)
        pb = pa.clone()
        wa, wb = ops.scenes_workspace(dev, S, Mmax, n), ops.scenes_workspace(dev, S, Mmax, n)
        ops.scenes_init(off_d, pa, wa, Mmax)
        ops.scenes_init(off_d, pb, wb, Mmax)
        ia, ib = (torch.full((B, n), -1, dtype=torch.int64, device=dev) for _ in range(2))
        sa, sb = (torch.full((B,), -1, dtype=torch.int64, device=dev) for _ in range(2))
        count = torch.zeros(T, dtype=torch.int32, device=dev)
        low = torch.zeros(S, dtype=torch.int32, device=dev)
        rows = torch.empty((B, n, 3), dtype=torch.float32, device=dev)
        first = torch.empty(B, dtype=torch.int32, device=dev)
        open_d = torch.empty(1, dtype=torch.int32, device=dev)
        seen, selected = set(), 0
        for k in range(4):
            ops.scenes_crop(xyz_d, pa, n, ia, sa, wa, S, Mmax, pad=True)
            ops.scenes_vote_crop(xyz_d, pb, count, low, 1000, n, rows, ib, sb, first, open_d, wb, S, Mmax, pad=True)
            assert torch.equal(sa, sb) and torch.equal(ia, ib), f"call {k}"
            assert torch.equal(pa.view(torch.int32), pb.view(torch.int32)), f"call {k}"
            assert int(open_d.item()) == S
            assert first.cpu().tolist() == [min(n, sizes[s]) for s in sb.cpu().tolist()]
            selected += int(first.sum().item())
            seen.update(sa.cpu().tolist())
        assert len(seen) > 1
        assert int(count.sum().item()) == selected          # once per selected point, the repeats not counted


@pytest.mark.parametrize("C,wide", [(13, 0), (2, 64)])
def test_scenes_vote_accumulate_bitwise_twin(C, wide):
    """Four slots in order: two crops of one scene that overlap, an idle slot (first = 0) whose logits are 1e30, and a padded
    crop (first < n) with 1e30 in its repeat slots.  The kernel takes no count at all."""
    from randlanet import _ops as ops
    from randlanet.utils import scene
    dev = _dev()
    rs = np.random.RandomState(3 + C)
    T, n, B = 4000, 1024, 4
    s, oms = scene.blend_factors(0.95)
    idx = np.stack([np.arange(100, 100 + n), np.arange(100 + n // 2, 100 + n // 2 + n), np.full(n, -1),
                    3000 + np.resize(np.arange(300), n)]).astype(np.int64)
    first = np.array([n, n, 0, 300], np.int32)
    prob = rs.uniform(0, 1, (T, C)).astype(np.float32)
    with torch.cuda.device(dev):
        prob_d = torch.from_numpy(prob).to(dev)
        idx_d, first_d = torch.from_numpy(idx).to(dev), torch.from_numpy(first).to(dev)
        for k in range(2):
            lg = (3 * rs.standard_normal((B, C, n + wide))).astype(np.float32)
            lg[2] = 1e30
            lg[3, 0, 300:] = 1e30
            before = prob.copy()
            for b in range(B):
                scene.scenes_vote_accumulate(prob, lg[b, :, :n], idx[b], oms, s, int(first[b]))
            ops.scenes_vote_accumulate(torch.from_numpy(lg).to(dev)[:, :, :n], idx_d, first_d, float(oms), float(s), prob_d)
            got = prob_d.cpu().numpy()
            assert np.array_equal(_bits(got), _bits(prob)), f"blend {k}"
            touched = np.zeros(T, bool)
            touched[100:100 + n // 2 + n] = True
            touched[3000:3300] = True
            assert np.array_equal(_bits(got[~touched]), _bits(before[~touched]))
            assert not np.array_equal(got[touched], before[touched])


# ----------------------------------------------------------------------------------- predict_scenes, evaluate_scenes
def _models(n_points, seed=0):
    """tests/test_scene_pad_gpu.py's pair: a GPU-placed model and a CPU-placed one with the same weights."""
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(seed)
    st = RandLANetSettings(n_classes=6, n_points=n_points, n_neighbors=8, layer_sizes=[16, 32])
    gpu = Model(st, use_gpu=True)
    assert gpu.device.type == "cuda"
    weights = {k: v.detach().cpu().clone() for k, v in gpu.module.state_dict().items()}
    cpu = Model(RandLANetSettings(**vars(st)), weights=weights, use_gpu=False)
    return gpu, cpu


def test_predict_scenes_gpu_matches_cpu_model():
    gpu, cpu = _models(4096, seed=1)
    rs = np.random.RandomState(4)
    scenes = [(rs.uniform(0, 10, (M, 3)).astype(np.float32), None) for M in (6000, 3000, 900)]
    kw = dict(votes=2, batch_size=2, seed=1, return_counts=True, return_info=True, pad_small_scenes=True)
    np.random.seed(21)
    out_g, cnt_g, info_g = gpu.predict_scenes(scenes, **kw)
    state_g = np.random.get_state()[1].copy()
    np.random.seed(21)
    out_c, cnt_c, info_c = cpu.predict_scenes(scenes, **kw)
    assert np.array_equal(np.random.get_state()[1], state_g)
    assert info_g["passes"] == info_c["passes"] and np.array_equal(info_g["crops"], info_c["crops"])
    assert info_g["crops"].sum() > 2 * info_g["passes"] - 2
    for (xyz, _), og, oc, cg, cc in zip(scenes, out_g, out_c, cnt_g, cnt_c):
        assert og.shape == (6, xyz.shape[0])
        assert np.array_equal(cg, cc), "different crop sequences"
        assert cg.min() >= 2
        assert np.abs(og - oc).max() < 1e-4
    assert np.all(cnt_g[1] == 2) and np.all(cnt_g[2] == 2)     # a scene below n: two whole-scene crops and out
    assert list(gpu.module._infer_steps) == [(2, 4096)]


@pytest.mark.parametrize("grid", [None, 0.25])
def test_evaluate_scenes_together_counts_raw_points_once(grid):
    from randlanet.utils import grid as grid_utils
    gpu, _ = _models(4096, seed=2)
    rs = np.random.RandomState(6)
    scenes = []
    for M in (6000, 900, 5000):
        labels = rs.randint(-1, 6, M)                   # -1: unlabelled
        scenes.append((rs.uniform(0, 10, (M, 3)).astype(np.float32), None, labels))
    kw = dict(batch_size=2, pad_small_scenes=True, grid=grid, seed=3)
    np.random.seed(0)
    out, conf = gpu.evaluate_scenes(scenes, return_confusion=True, together=True, **kw)
    np.random.seed(0)
    probs = gpu.predict_scenes(scenes, **kw)
    want = sum(grid_utils.confusion(np.ascontiguousarray(p.T), l, 6) for p, (_, _, l) in zip(probs, scenes))
    assert conf.sum() == sum(int((l >= 0).sum()) for _, _, l in scenes)
    assert np.array_equal(conf, want)
    assert 0.0 <= out["OA"] <= 1.0
    assert list(gpu.module._infer_steps) == [(2, 4096)]
