"""Model.train_scenes without a GPU: the multi-scene crop twin (utils/scene.py scenes_*) against restatements of
RandLA-Net's training sampler, the host draws of the scene crop loader, argument errors, and the host-side checks of the
rl_scenes_* entry points."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scenes_xyz(rs, sizes, lattice):
    parts = []
    for M in sizes:
        if lattice:             # many equal distances, duplicated points
            x = np.floor(rs.uniform(0, 5, (M, 3))).astype(np.float32) * np.float32(0.5)
            x[rs.randint(0, M, M // 4)] = x[rs.randint(0, M, M // 4)]
        else:
            x = rs.uniform(-2, 2, (M, 3)).astype(np.float32)
        parts.append(x)
    return np.concatenate(parts)


def _tied_possibility(rs, T):
    """Few distinct values: heavy ties inside and across scenes."""
    return rs.randint(0, 3, T).astype(np.float32) * np.float32(0.25)


def test_pick_is_the_two_level_pick():
    """argmin over (possibility, row) of all scenes == the argmin of the scenes' minima, then the argmin inside the scene
    (the authors' spatially_regular_gen), ties to the lower index at both levels."""
    from randlanet.utils import scene
    rs = np.random.RandomState(0)
    for _ in range(200):
        sizes = rs.randint(1, 40, rs.randint(1, 9))
        off = scene.scene_offsets(sizes)
        poss = _tied_possibility(rs, int(off[-1]))
        mins = [poss[off[s]:off[s + 1]].min() for s in range(len(sizes))]
        s_ref = int(np.argmin(mins))
        g_ref = int(off[s_ref] + np.argmin(poss[off[s_ref]:off[s_ref + 1]]))
        assert scene.scenes_pick(poss, off) == (g_ref, s_ref)


@pytest.mark.parametrize("noise", [0.0, 0.3])
@pytest.mark.parametrize("lattice", [False, True])
def test_twin_crop_is_the_lexsort_prefix_inside_the_picked_scene(noise, lattice):
    from randlanet.utils import scene
    rs = np.random.RandomState(7 + lattice)
    sizes = [150, 400, 64, 999]
    n = 64
    xyz = _scenes_xyz(rs, sizes, lattice)
    off = scene.scene_offsets(sizes)
    poss = _tied_possibility(rs, xyz.shape[0]) if lattice else scene.initial_possibility(xyz.shape[0], seed=3)
    np.random.seed(11)
    for _ in range(12):
        before = poss.copy()
        g, s = scene.scenes_pick(poss, off)
        c = scene.centre_noise(noise)
        p = xyz[g] + c
        b, e = off[s], off[s + 1]
        d = p - xyz[b:e]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        want = np.sort(np.lexsort((np.arange(e - b), d2))[:n]) + b
        s_got, idx = scene.scenes_crop(xyz, off, poss, n, c if noise > 0 else None)
        assert s_got == s and np.array_equal(idx, want)
        dmax = d2[want - b].max()
        t = np.float32(1) - (d2[want - b] / dmax if dmax > 0 else np.zeros(n, np.float32))
        expect = before.copy()
        expect[want] = before[want] + t * t
        assert np.array_equal(poss.view(np.uint32), expect.view(np.uint32))


def test_one_scene_without_noise_is_predict_scenes_crop():
    from randlanet.utils import scene
    rs = np.random.RandomState(1)
    xyz = _scenes_xyz(rs, [2000], lattice=True)
    p1 = scene.initial_possibility(2000, seed=0)
    p2 = p1.copy()
    off = scene.scene_offsets([2000])
    for _ in range(10):
        s, idx = scene.scenes_crop(xyz, off, p1, 300)
        assert s == 0 and np.array_equal(idx, scene.crop(xyz, p2, 300))
        assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32))


@pytest.mark.parametrize("noise", [0.0, 0.5])
@pytest.mark.parametrize("jitter_on_host", [False, True])
def test_host_draws_per_crop(noise, jitter_on_host):
    """Three normals per crop for the centre when center_noise > 0 and none otherwise, then the augmentation draws in the
    device loader's order; torch's generator untouched."""
    from randlanet.utils.augmentation import AugmentationSettings, _rotation
    from randlanet.utils.scene_loader import crop_draws
    a = AugmentationSettings()
    n = 50
    torch_state = torch.get_rng_state()
    np.random.seed(5)
    got = [crop_draws(n, noise, a, jitter_on_host) for _ in range(3)]
    probe = np.random.rand()
    np.random.seed(5)
    for centre, aug in got:
        if noise > 0:
            assert np.array_equal(centre, np.random.normal(0, noise, 3).astype(np.float32))
        else:
            assert np.array_equal(centre, np.zeros(3, np.float32))
        if jitter_on_host:
            assert np.array_equal(aug["jitter"], np.random.randn(n, 3))
        else:
            assert aug["jitter"] is None
        assert aug["scale"] == np.random.uniform(1 - a.scale_limit, 1 + a.scale_limit)
        angles = [float(np.clip(s * np.random.randn(), -lim, lim))
                  for s, lim in zip(a.rotation_angle_variances, a.rotation_angle_limits)]
        assert np.array_equal(aug["R"], _rotation(*angles))
        assert np.array_equal(aug["shift"], np.random.uniform(-a.shift_limit, a.shift_limit, 3))
    assert probe == np.random.rand()                       # nothing else was drawn
    assert torch.equal(torch.get_rng_state(), torch_state)
    # without augmentation: the centre noise only
    np.random.seed(9)
    centre, aug = crop_draws(n, noise, None, jitter_on_host)
    probe = np.random.rand()
    np.random.seed(9)
    if noise > 0:
        np.random.normal(0, noise, 3)
    assert aug is None and probe == np.random.rand()


def _scene(M, F=1, seed=0):
    rs = np.random.RandomState(seed)
    return (rs.uniform(0, 1, (M, 3)), rs.uniform(0, 1, (M, F)).astype(np.float32), rs.randint(0, 3, M).astype(np.int64))


def test_argument_errors():
    from randlanet.utils.scene_loader import get_scene_crop_loader
    with pytest.raises(ValueError, match=r"scene 1 has 99 points"):
        get_scene_crop_loader([_scene(200), _scene(99)], 100, 2, 4, device="cpu")
    with pytest.raises(ValueError, match=r"scene 1: 2 features"):
        get_scene_crop_loader([_scene(200), _scene(200, F=2)], 100, 2, 4, device="cpu")
    x, f, l = _scene(200)
    with pytest.raises(ValueError, match="labels"):
        get_scene_crop_loader([(x, f, l[:, None])], 100, 2, 4, device="cpu")
    with pytest.raises(ValueError, match="labels"):
        get_scene_crop_loader([(x, f, l[:150])], 100, 2, 4, device="cpu")
    with pytest.raises(ValueError, match="xyz"):
        get_scene_crop_loader([(x[:, :2], f, l)], 100, 2, 4, device="cpu")


def test_loader_and_train_scenes_need_a_gpu():
    from randlanet._hip import HipKernelError
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    from randlanet.utils.scene_loader import get_scene_crop_loader
    from randlanet.utils.trainer import TrainingSettings
    with pytest.raises(HipKernelError, match="needs a GPU"):
        get_scene_crop_loader([_scene(200)], 100, 2, 4, device="cpu")
    model = Model(RandLANetSettings(n_classes=3, n_features=1, n_points=128, n_neighbors=4, layer_sizes=[16, 32]),
                  use_gpu=False)
    with pytest.raises(HipKernelError, match="train_scenes trains on the GPU"):
        model.train_scenes([_scene(300)], [_scene(300)], TrainingSettings(epochs=1, batch_size=2), crops_per_epoch=4,
                           validation_crops=2, class_names=["a", "b", "c"])


@pytest.fixture(scope="module")
def lib():
    from randlanet import _hip
    if not os.path.exists(_hip.library_path()):
        subprocess.check_call(["make", "-C", os.path.join(REPO, "3d_recognizer_amd", "csrc"), "-j4"])
    return _hip.lib()


def test_scenes_symbols_are_exported(lib):
    from randlanet import _hip
    raw = ctypes.CDLL(_hip.library_path())
    for name in ("rl_scenes_workspace_bytes", "rl_scenes_init", "rl_scenes_crop"):
        assert name in _hip.EXPORTS and hasattr(raw, name)
    assert lib.rl_version() == 110


def test_scenes_argument_errors_on_the_host(lib):
    from randlanet import _hip
    S, Mmax, n, B = 4, 1000, 100, 3
    need = lib.rl_scenes_workspace_bytes(S, Mmax, n)
    assert need >= 4 * Mmax + 8 * S and lib.rl_scenes_workspace_bytes(0, Mmax, n) == 0
    assert lib.rl_scenes_workspace_bytes(S, 0, n) == 0
    fake = 1 << 20              # never dereferenced: every call below is refused before a launch
    assert lib.rl_scenes_init(fake, 0, Mmax, fake, fake, need, None) == _hip.ERR_ARGS
    assert lib.rl_scenes_init(fake, S, Mmax, fake, fake, need - 1, None) == _hip.ERR_ARGS
    assert b"workspace" in lib.rl_last_error()
    assert lib.rl_scenes_init(None, S, Mmax, fake, fake, need, None) == _hip.ERR_ARGS
    assert lib.rl_scenes_init(fake, S, Mmax, fake, fake + 16, need, None) == _hip.ERR_ARGS
    assert lib.rl_scenes_crop(fake, 3, S, Mmax, fake, Mmax + 1, B, None, fake, fake, fake, need, None) == _hip.ERR_ARGS
    assert b"n=1001" in lib.rl_last_error()
    assert lib.rl_scenes_crop(fake, 2, S, Mmax, fake, n, B, None, fake, fake, fake, need, None) == _hip.ERR_ARGS
    assert b"stride=2" in lib.rl_last_error()
    assert lib.rl_scenes_crop(fake, 3, S, Mmax, fake, n, 0, None, fake, fake, fake, need, None) == _hip.ERR_ARGS
    assert lib.rl_scenes_crop(fake, 3, S, Mmax, fake, n, B, None, fake, fake, fake, need - 1, None) == _hip.ERR_ARGS
    assert b"workspace" in lib.rl_last_error()
    assert lib.rl_scenes_crop(fake, 3, S, Mmax, fake, n, B, None, None, fake, fake, need, None) == _hip.ERR_ARGS
    assert lib.rl_scenes_crop(fake, 3, S, 1 << 31, fake, n, B, None, fake, fake, fake, need, None) == _hip.ERR_ARGS
