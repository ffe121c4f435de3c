"""Padded crops (pad_small_scenes) on the MI355X: rl_scenes_crop_padded, rl_scene_crop_padded and rl_scene_accumulate_first
against their numpy twins (utils/scene.py) bit for bit and against the unpadded entries where no scene is small, the scene
crop loader against a host restatement, and train_scenes / predict_scene / evaluate_scenes with scenes below n_points."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 4096                    # the crop size of the kernel tests


def _dev():
    return torch.device("cuda", 0)


def _lattice(rs, M):
    """Coarse lattice (many equal distances) with a quarter of the points duplicated, as tests/test_scene_train_gpu.py."""
    ext = max(4.0, round(M ** (1 / 3)))
    x = np.floor(rs.uniform(0, ext, (M, 3))).astype(np.float32) * np.float32(0.25)
    if M >= 4:
        x[rs.randint(0, M, M // 4)] = x[rs.randint(0, M, M // 4)]
    return x


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# above n, at n, one below, not dividing n, one point past a 256-thread tile, one wavefront, a single point
SIZES = [6000, 4096, 4095, 1365, 257, 64, 1]


@pytest.mark.parametrize("noise", [0.0, 0.05])
def test_scenes_crop_padded_bitwise_twin(noise):
    from randlanet import _ops as ops
    from randlanet.utils import scene
    rs = np.random.RandomState(7)
    sizes, n, B, calls = SIZES, N, 4, 5
    xyz = np.concatenate([_lattice(rs, M) for M in sizes])
    T = xyz.shape[0]
    off = scene.scene_offsets(sizes)
    poss = scene.initial_possibility(T, seed=5)
    poss = (np.floor(poss * np.float32(4000)) * np.float32(2.5e-4)).astype(np.float32)     # equal possibilities too
    for s in range(len(sizes)):            # the later (smaller) a scene, the lower its possibilities: each is picked early
        poss[off[s]:off[s + 1]] *= np.float32(0.5 ** s)
    dev = _dev()
    S, Mmax = len(sizes), max(sizes)
    seen = set()
    with torch.cuda.device(dev):
        xyz_d = torch.from_numpy(xyz).to(dev)
        poss_d = torch.from_numpy(poss).to(dev)
        ws = ops.scenes_workspace(dev, S, Mmax, n)
        ops.scenes_init(torch.from_numpy(off).to(dev), poss_d, ws, Mmax)
        for k in range(calls):
            nz = rs.normal(0, noise, (B, 3)).astype(np.float32) if noise > 0 else None
            want = [scene.scenes_crop(xyz, off, poss, n, None if nz is None else nz[b], pad=True) for b in range(B)]
            idx = torch.full((B, n), -1, dtype=torch.int64, device=dev)
            sc = torch.full((B,), -1, dtype=torch.int64, device=dev)
            ops.scenes_crop(xyz_d, poss_d, n, idx, sc, ws, S, Mmax, None if nz is None else torch.from_numpy(nz).to(dev),
                            pad=True)
            assert sc.cpu().tolist() == [s for s, _ in want], f"call {k}: scenes differ"
            got = idx.cpu().numpy()
            for b in range(B):
                assert np.array_equal(got[b], want[b][1]), f"call {k}, crop {b}: indices differ"
            assert np.array_equal(_bits(poss_d.cpu().numpy()), _bits(poss)), f"call {k}: possibilities differ"
            seen.update(s for s, _ in want)
    assert seen == set(range(S)), seen


def test_scenes_crop_padded_with_n_above_every_scene():
    """n above max_points: the old entry refuses it, the padded one repeats every scene."""
    from randlanet import _hip as H
    from randlanet import _ops as ops
    from randlanet.utils import scene
    rs = np.random.RandomState(3)
    sizes, n, B = [1000, 300, 2500], N, 3
    xyz = np.concatenate([_lattice(rs, M) for M in sizes])
    off = scene.scene_offsets(sizes)
    poss = scene.initial_possibility(xyz.shape[0], seed=1)
    dev = _dev()
    S, Mmax = len(sizes), max(sizes)
    with torch.cuda.device(dev):
        xyz_d = torch.from_numpy(xyz).to(dev)
        poss_d = torch.from_numpy(poss).to(dev)
        ws = ops.scenes_workspace(dev, S, Mmax, n)
        ops.scenes_init(torch.from_numpy(off).to(dev), poss_d, ws, Mmax)
        idx = torch.full((B, n), -1, dtype=torch.int64, device=dev)
        sc = torch.full((B,), -1, dtype=torch.int64, device=dev)
        with pytest.raises(H.HipKernelError, match="crop of n=4096 points, largest scene 2500"):
            ops.scenes_crop(xyz_d, poss_d, n, idx, sc, ws, S, Mmax)
        for k in range(2):
            want = [scene.scenes_crop(xyz, off, poss, n, pad=True) for _ in range(B)]
            ops.scenes_crop(xyz_d, poss_d, n, idx, sc, ws, S, Mmax, pad=True)
            assert sc.cpu().tolist() == [s for s, _ in want]
            assert np.array_equal(idx.cpu().numpy(), np.stack([i for _, i in want]))
            assert np.array_equal(_bits(poss_d.cpu().numpy()), _bits(poss))


@pytest.mark.parametrize("M,F,extra", [(4095, 0, 0), (1000, 3, 2), (63, 0, 1), (63, 3, 0)])
def test_scene_crop_padded_bitwise_twin(M, F, extra):
    from randlanet import _hip as H
    from randlanet import _ops as ops
    from randlanet.utils import scene
    dev = _dev()
    n = N
    rs = np.random.RandomState(M + F)
    xyz = _lattice(rs, M)
    cloud = np.concatenate([xyz, rs.standard_normal((M, F)).astype(np.float32)], axis=1) if F else xyz
    dim = 3 + F
    poss = scene.initial_possibility(M, seed=F)
    if F:                   # equal possibilities too: the pick must break ties by the lowest index
        poss = (np.floor(poss * np.float32(4000)) * np.float32(2.5e-4)).astype(np.float32)
    with torch.cuda.device(dev):
        cloud_d = torch.from_numpy(cloud).to(dev)
        poss_d = torch.from_numpy(poss).to(dev)
        ws = ops.scene_workspace(dev, M, n)
        rows = torch.full((n, dim + extra), -7.0, dtype=torch.float32, device=dev)
        idx = torch.full((n,), -1, dtype=torch.int32, device=dev)
        with pytest.raises(H.HipKernelError, match=f"rl_scene_crop: crop of n={n} points out of M={M}"):
            ops.scene_crop(cloud_d, poss_d, n, rows, idx, ws)
        for k in range(4):
            want = scene.crop(cloud, poss, n, pad=True)
            ops.scene_crop(cloud_d, poss_d, n, rows, idx, ws, pad=True)
            assert np.array_equal(idx.cpu().numpy(), want), f"crop {k}: indices differ"
            assert np.array_equal(want, np.resize(np.arange(M), n))
            r = rows.cpu().numpy()
            assert np.array_equal(_bits(r[:, :dim]), _bits(cloud[want])), f"crop {k}: rows differ"
            assert np.all(r[:, dim:] == -7.0)
            assert np.array_equal(_bits(poss_d.cpu().numpy()), _bits(poss)), f"crop {k}: possibilities differ"


def test_padded_entries_equal_the_old_entries_on_large_scenes():
    from randlanet import _ops as ops
    from randlanet.utils import scene
    dev = _dev()
    rs = np.random.RandomState(11)
    n = N
    sizes = [6000, 4096, 20000, 4097]
    xyz = np.concatenate([_lattice(rs, M) for M in sizes])
    off = scene.scene_offsets(sizes)
    poss = scene.initial_possibility(xyz.shape[0], seed=4)
    poss[off[1]:off[2]] *= np.float32(0.0625)
    S, Mmax, B = len(sizes), max(sizes), 4
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
        seen = set()
        for k in range(4):
            nz = torch.from_numpy(rs.normal(0, 0.05, (B, 3)).astype(np.float32)).to(dev) if k % 2 else None
            ops.scenes_crop(xyz_d, pa, n, ia, sa, wa, S, Mmax, nz)
            ops.scenes_crop(xyz_d, pb, n, ib, sb, wb, S, Mmax, nz, pad=True)
            assert torch.equal(sa, sb) and torch.equal(ia, ib), f"call {k}"
            assert torch.equal(pa.view(torch.int32), pb.view(torch.int32)), f"call {k}"
            seen.update(sa.cpu().tolist())
        assert len(seen) > 1
        # one scene, rl_scene_crop against rl_scene_crop_padded: M above n and M == n
        for M in (20000, n):
            cloud = np.concatenate([_lattice(rs, M), rs.standard_normal((M, 2)).astype(np.float32)], axis=1)
            cloud_d = torch.from_numpy(cloud).to(dev)
            pa = torch.from_numpy(scene.initial_possibility(M, 1)).to(dev)
            pb = pa.clone()
            ws = ops.scene_workspace(dev, M, n)
            ra, rb = (torch.full((n, 6), -7.0, dtype=torch.float32, device=dev) for _ in range(2))
            ja, jb = (torch.full((n,), -1, dtype=torch.int32, device=dev) for _ in range(2))
            for k in range(4):
                ops.scene_crop(cloud_d, pa, n, ra, ja, ws)
                ops.scene_crop(cloud_d, pb, n, rb, jb, ws, pad=True)
                assert torch.equal(ja, jb) and torch.equal(ra.view(torch.int32), rb.view(torch.int32)), f"M={M} crop {k}"
                assert torch.equal(pa.view(torch.int32), pb.view(torch.int32)), f"M={M} crop {k}"


def test_scene_accumulate_first_bitwise_twin():
    from randlanet import _ops as ops
    from randlanet.utils import scene
    dev = _dev()
    rs = np.random.RandomState(3)
    M, C, n, first = 1000, 13, N, 1000
    s, oms = scene.blend_factors(0.95)
    prob = np.zeros((M, C), np.float32)
    count = np.zeros(M, np.int32)
    idx = np.resize(np.arange(M), n).astype(np.int32)
    with torch.cuda.device(dev):
        prob_d = torch.zeros((M, C), dtype=torch.float32, device=dev)
        count_d = torch.zeros(M, dtype=torch.int32, device=dev)
        idx_d = torch.from_numpy(idx).to(dev)
        for k in range(3):                  # blended over itself: s*prob + (1-s)*softmax on non-zero prob as well
            lg = (3 * rs.standard_normal((C, n))).astype(np.float32)
            scene.accumulate(prob, count, lg, idx, oms, s, first=first)
            ops.scene_accumulate(torch.from_numpy(lg).to(dev), idx_d, float(oms), float(s), prob_d, count_d, first=first)
            got = prob_d.cpu().numpy()
            differ = int((_bits(got) != _bits(prob)).sum())
            rel = float((np.abs(got.astype(np.float64) - prob) / np.maximum(np.abs(prob), 1e-30)).max())
            print(f"accumulate_first blend {k}: {differ} of {got.size} probabilities differ in their bits, "
                  f"largest relative difference {rel:.3e}")
            assert np.array_equal(count_d.cpu().numpy(), count) and np.all(count == k + 1)
            assert differ == 0


def test_scene_accumulate_first_bitwise_twin_wide_logits():
    """As above on logits whose spread passes every branch of the fixed exp: differences to the column's largest logit
    beyond -87 (the result is 0), exactly -87, and -inf logits."""
    from randlanet import _ops as ops
    from randlanet.utils import scene
    dev = _dev()
    rs = np.random.RandomState(6)
    M, C, n, first = 1000, 13, N, 1000
    s, oms = scene.blend_factors(0.95)
    lg = (40 * rs.standard_normal((C, n))).astype(np.float32)
    lg[3, ::7] = -np.inf
    lg[:, 5] = 0
    lg[1, 5] = -87
    lg[2, 5] = np.nextafter(np.float32(-87), np.float32(-100))
    prob = rs.uniform(0, 1, (M, C)).astype(np.float32)
    count = np.zeros(M, np.int32)
    idx = np.resize(np.arange(M), n).astype(np.int32)
    with torch.cuda.device(dev):
        prob_d, count_d = torch.from_numpy(prob).to(dev), torch.from_numpy(count).to(dev)
        scene.accumulate(prob, count, lg, idx, oms, s, first=first)
        ops.scene_accumulate(torch.from_numpy(lg).to(dev), torch.from_numpy(idx).to(dev), float(oms), float(s), prob_d, count_d,
                             first=first)
        assert np.array_equal(count_d.cpu().numpy(), count)
        assert np.array_equal(_bits(prob_d.cpu().numpy()), _bits(prob))


def test_scene_accumulate_first_leaves_the_other_slots_untouched():
    from randlanet import _ops as ops
    dev = _dev()
    rs = np.random.RandomState(4)
    M, C, n, first = 2000, 13, N, 1000
    with torch.cuda.device(dev):
        prob_d = torch.from_numpy(rs.uniform(0, 1, (M, C)).astype(np.float32)).to(dev)
        count_d = torch.from_numpy(rs.randint(0, 5, M).astype(np.int32)).to(dev)
        before_p, before_c = prob_d.clone(), count_d.clone()
        # the leading 1000 slots point at rows 0 .. 999, the others (logits of 1e30 in class 0) at rows 1000 .. 1999
        idx = np.concatenate([np.arange(first), first + np.resize(np.arange(1000), n - first)]).astype(np.int32)
        lg = (3 * rs.standard_normal((C, n))).astype(np.float32)
        lg[0, first:] = 1e30
        lg_d, idx_d = torch.from_numpy(lg).to(dev), torch.from_numpy(idx).to(dev)
        ops.scene_accumulate(lg_d, idx_d, 0.05, 0.95, prob_d, count_d, first=first)
        assert torch.equal(prob_d[first:].view(torch.int32), before_p[first:].view(torch.int32))
        assert torch.equal(count_d[first:], before_c[first:]) and torch.equal(count_d[:first], before_c[:first] + 1)
        assert not torch.equal(prob_d[:first], before_p[:first])
        # a strided view: the leading (C, 1000) columns of the (C, 4096) logits, blended whole, against a packed copy
        p1, c1 = before_p.clone(), before_c.clone()
        ops.scene_accumulate(lg_d[:, :first], idx_d[:first].contiguous(), 0.05, 0.95, p1, c1, first=first)
        assert torch.equal(p1.view(torch.int32), prob_d.view(torch.int32)) and torch.equal(c1, count_d)


def test_scene_accumulate_first_is_close_to_rl_scene_accumulate():
    """The first-slots entry against the old entry on the leading columns copied out.  Their softmax differs in the exp
    alone (a fixed float32 expression against the library's expf), so the counts are equal and the probabilities agree
    within the 1e-6 that tests/test_scene_gpu.py holds rl_scene_accumulate to against np.exp."""
    from randlanet import _ops as ops
    dev = _dev()
    rs = np.random.RandomState(5)
    M, C, n, first = 1000, 13, N, 1000
    with torch.cuda.device(dev):
        idx = torch.from_numpy(np.resize(np.arange(M), n).astype(np.int32)).to(dev)
        pa = torch.zeros((M, C), dtype=torch.float32, device=dev)
        pb = pa.clone()
        ca = torch.zeros(M, dtype=torch.int32, device=dev)
        cb = ca.clone()
        for k in range(3):
            lg = torch.from_numpy((3 * rs.standard_normal((C, n))).astype(np.float32)).to(dev)
            ops.scene_accumulate(lg, idx, 0.05, 0.95, pa, ca, first=first)
            ops.scene_accumulate(lg[:, :first].contiguous(), idx[:first].contiguous(), 0.05, 0.95, pb, cb)
            assert torch.equal(ca, cb)
            assert bool(((pa - pb).abs() <= 1e-6 * pb.abs() + 1e-12).all())


# ------------------------------------------------------------------------------------------------------------ loader
def _close(got, want):
    """tests/test_pipeline_gpu.py's tolerance: one float32 ulp of the value (or of the extent near zero), few differ."""
    scale = max(1.0, float(np.abs(want).max()))
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.maximum(np.spacing(np.abs(want).astype(np.float32)), np.spacing(np.float32(scale))).astype(np.float64)
    return bool((diff <= ulp).all()) and float((diff > 0).mean()) < 0.05


@pytest.mark.parametrize("noise", [0.0, 0.3])
def test_padded_loader_batches_match_a_host_restatement(noise):
    from randlanet.utils import scene
    from randlanet.utils.augmentation import AugmentationSettings, perturbate_point_cloud
    from randlanet.utils.scene_loader import get_scene_crop_loader
    rs = np.random.RandomState(12)
    sizes, n, B, crops = [5000, 900, 3000], 2048, 3, 7
    scenes = [(rs.uniform(0, 4, (M, 3)), rs.standard_normal((M, 2)).astype(np.float32),
               rs.randint(0, 5, M).astype(np.int64)) for M in sizes]
    aug = AugmentationSettings()
    with pytest.raises(ValueError, match="scene 1 has 900 points, fewer than the crop size n=2048"):
        get_scene_crop_loader(scenes, n, B, crops, device="cuda")
    np.random.seed(4)
    loader = get_scene_crop_loader(scenes, n, B, crops, center_noise=noise, augmentation_settings=aug, seed=2,
                                   device="cuda", pad_small_scenes=True)
    got = [(i.cpu().numpy(), lab.cpu().numpy(), s.cpu().numpy()) for i, lab, s in loader]
    after = np.random.get_state()[1].copy()
    assert [g[0].shape for g in got] == [(3, n, 5), (3, n, 5), (1, n, 5)]
    np.random.seed(4)
    xyz = np.concatenate([x.astype(np.float32) for x, _, _ in scenes])
    feat = np.concatenate([f for _, f, _ in scenes])
    lab = np.concatenate([l for _, _, l in scenes])
    off = scene.scene_offsets(sizes)
    poss = scene.initial_possibility(xyz.shape[0], 2)
    picked = []
    for inp, lb, sc in got:
        for b in range(inp.shape[0]):
            c = scene.centre_noise(noise)
            s, idx = scene.scenes_crop(xyz, off, poss, n, c if noise > 0 else None, pad=True)
            want = perturbate_point_cloud(xyz[idx], aug).astype(np.float32)       # (jitter per slot: n draws)
            assert sc[b] == s
            assert np.array_equal(lb[b], lab[idx])
            assert np.array_equal(inp[b][:, 3:], feat[idx])
            assert _close(inp[b][:, :3], want)
            picked.append(s)
    assert 1 in picked, picked
    assert np.array_equal(np.random.get_state()[1], after)
    assert np.array_equal(_bits(loader.possibility.cpu().numpy()), _bits(poss))


# ------------------------------------------------------------------------------------------------------ train_scenes
def _labelled_scene(rs, M, extent=3.0):
    xyz = rs.uniform((0, 0, -1), (extent, extent, 1), (M, 3)).astype(np.float32)
    return xyz, np.zeros((M, 0), np.float32), (xyz[:, 2] > 0).astype(np.int64)


def _train(train, val, **kw):
    from randlanet import AugmentationSettings, Model, RandLANetSettings, TrainingSettings
    torch.manual_seed(0)
    np.random.seed(0)
    model = Model(RandLANetSettings(n_classes=2, n_points=2048, n_neighbors=8, layer_sizes=[8, 16, 32, 32]))
    hist = []
    model.train_scenes(train, val, TrainingSettings(epochs=2, batch_size=4, learning_rate=1e-2, early_stopping=False),
                       AugmentationSettings(), crops_per_epoch=10, validation_crops=4, center_noise=0.05, seed=3,
                       class_names=["below", "above"], callbacks=[lambda e, m: hist.append(m["loss"])], **kw)
    return model, hist


def test_train_scenes_with_small_scenes():
    rs = np.random.RandomState(8)
    train = [_labelled_scene(rs, M) for M in (6000, 1500, 700)]
    val = [_labelled_scene(rs, 1800)]
    with pytest.raises(ValueError, match="scene 1 has 1500 points, fewer than the crop size n=2048"):
        _train(train, val)
    m1, h1 = _train(train, val, pad_small_scenes=True)
    m2, h2 = _train(train, val, pad_small_scenes=True)
    assert len(h1) == 2 and np.all(np.isfinite(h1)), h1
    for (k, a), b in zip(m1.module.state_dict().items(), m2.module.state_dict().values()):
        assert torch.equal(a, b), k
    assert h1 == h2


def test_train_scenes_grid_with_a_scene_below_n_points_cells():
    rs = np.random.RandomState(9)
    # 0.25-edge cells over 3 x 3 x 2: at most 12 * 12 * 8 = 1152 cells < 2048; the large scene spans 8 x 8 x 2 (8192 cells)
    train = [_labelled_scene(rs, 30000, extent=8.0), _labelled_scene(rs, 5000)]
    val = [_labelled_scene(rs, 30000, extent=8.0)]
    with pytest.raises(ValueError, match=r"scene 1 has \d+ points, fewer than the crop size n=2048"):
        _train(train, val, grid=0.25)
    _, h = _train(train, val, grid=0.25, pad_small_scenes=True)
    assert len(h) == 2 and np.all(np.isfinite(h)), h


# ----------------------------------------------------------------------------------- predict_scene, evaluate_scenes
def _models(n_points, seed=0):
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(seed)
    st = RandLANetSettings(n_classes=6, n_points=n_points, n_neighbors=8, layer_sizes=[16, 32])
    gpu = Model(st, use_gpu=True)
    assert gpu.device.type == "cuda"
    weights = {k: v.detach().cpu().clone() for k, v in gpu.module.state_dict().items()}
    cpu = Model(RandLANetSettings(**vars(st)), weights=weights, use_gpu=False)
    return gpu, cpu


def test_predict_scene_padded_gpu_matches_cpu_model():
    gpu, cpu = _models(4096, seed=1)
    xyz = np.random.RandomState(4).uniform(0, 10, (3000, 3)).astype(np.float32)
    np.random.seed(21)
    out_g, cnt_g = gpu.predict_scene(xyz, votes=2, batch_size=2, seed=1, return_counts=True, pad_small_scenes=True)
    state_g = np.random.get_state()[1].copy()
    np.random.seed(21)
    out_c, cnt_c = cpu.predict_scene(xyz, votes=2, batch_size=2, seed=1, return_counts=True, pad_small_scenes=True)
    assert np.array_equal(np.random.get_state()[1], state_g)
    assert out_g.shape == (6, 3000)
    assert np.array_equal(cnt_g, cnt_c), "different crop sequences"
    assert np.all(cnt_g == 2)               # one pass of two whole-scene crops, each point voted once per crop
    assert np.abs(out_g - out_c).max() < 1e-4
    assert list(gpu.module._infer_steps) == [(2, 4096)]


def test_evaluate_scenes_padded_counts_raw_points_once_with_one_forward_shape():
    gpu, _ = _models(4096, seed=2)
    rs = np.random.RandomState(6)
    scenes = []
    for M in (6000, 900):
        labels = rs.randint(-1, 6, M)                   # -1: unlabelled
        scenes.append((rs.uniform(0, 10, (M, 3)).astype(np.float32), None, labels))
    np.random.seed(0)
    out, conf = gpu.evaluate_scenes(scenes, batch_size=2, return_confusion=True, pad_small_scenes=True)
    assert conf.sum() == sum(int((l >= 0).sum()) for _, _, l in scenes)
    assert 0.0 <= out["OA"] <= 1.0
    assert list(gpu.module._infer_steps) == [(2, 4096)]
