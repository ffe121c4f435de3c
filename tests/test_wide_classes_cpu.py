"""33 .. 256 classes, the part that needs no GPU: the library and its new symbol, the refusal above RL_MAX_CLASSES made before
any step, the recipe of the wide tests, and the YARDSTICK's own error - the GPU tests (test_wide_classes_gpu.py) hold the
kernels to the bounds of the masked-loss tests (loss 2e-6 * max(1, |loss|), gradient 1e-4 * max|ref| + 1e-9), which is only a
statement about the kernels if the yardstick's fp32 run sits far inside them: asserted here at a third of each bound."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import masked_inputs as MI
import wide_inputs as WI

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from randlanet import _hip
    if not os.path.exists(_hip.library_path()):
        subprocess.check_call(["make", "-C", os.path.join(REPO, "3d_recognizer_amd", "csrc"), "-j4"])
    return _hip.lib()


def test_library_loads_and_exports_the_class_bound(lib):
    from randlanet import _hip
    raw = ctypes.CDLL(_hip.library_path())
    assert "rl_loss_max_classes" in _hip.EXPORTS and hasattr(raw, "rl_loss_max_classes")
    assert lib.rl_version() == _hip.ABI_VERSION == 110
    assert lib.rl_loss_max_classes() == _hip.MAX_LOSS_CLASSES == 256
    header = open(os.path.join(REPO, "include", "rl_randlanet.h")).read()
    assert "#define RL_MAX_CLASSES 256" in header
    # the work buffer and the totals record keep their layout at every class count
    for C in (32, 33, 256):
        assert lib.rl_loss_totals_offset(C) == 1024 * (5 * C + 1)
        assert lib.rl_loss_work_doubles(1, C) == 1025 * (5 * C + 1)
    # the fused head stays at 32 classes
    assert lib.rl_head_supported(32, 32) == 1 and lib.rl_head_supported(33, 32) == 0


@pytest.mark.parametrize("C", WI.CLASSES)
def test_recipe(C):
    labels = WI.inputs(C)[1]
    WI.check_recipe(labels, C)
    assert not (set(WI.MARKS(C)) & set(range(C)))           # no mark is a class (255 would be one at C = 256)
    assert WI.base_labels(WI.B, WI.N, C).min() == 0 and WI.base_labels(WI.B, WI.N, C).max() == C - 1


@pytest.mark.parametrize("mode", WI.MODES)
@pytest.mark.parametrize("C", WI.CLASSES)
def test_the_yardsticks_own_fp32_error_is_a_third_of_the_bounds(C, mode):
    logits, labels, w = WI.mode_inputs(C, mode)
    worst_l = worst_g = 0.0
    for name in MI.LOSS_NAMES:
        l64, g64 = WI.yardstick(name, logits, labels, w)
        l32, g32 = WI.yardstick(name, logits, labels, w, torch.float32)
        e_l, e_g = abs(l32 - l64), float(np.abs(g32 - g64).max())
        worst_l, worst_g = max(worst_l, e_l / max(1.0, abs(l64))), max(worst_g, e_g / np.abs(g64).max())
        assert e_l <= 2e-6 * max(1.0, abs(l64)) / 3, (name, l32, l64)
        assert e_g <= (1e-4 * np.abs(g64).max() + 1e-9) / 3, (name, e_g, np.abs(g64).max())
    print(f"[wide yardstick] C={C} {mode}: fp32 vs fp64 loss {worst_l:.1e}, relative gradient {worst_g:.1e}")


@pytest.mark.parametrize("name", sorted(WI.TVERSKY))
def test_tversky_twin_is_the_oracle_where_the_oracle_speaks(name):
    """tversky_twin with the background neglected is the oracle's loss (which always neglects it): the twin's other half,
    the background kept, rests on the same lines.  On the input with empty classes."""
    from oracle.loss_metrics_oracle import loss_by_name
    logits, labels = WI.empty_class_inputs()
    assert labels.max() == 31 and logits.shape[1] == 64
    lg = torch.from_numpy(logits).double().requires_grad_(True)
    ref = loss_by_name(name, lg, torch.from_numpy(labels))
    ref.backward()
    loss, grad = WI.tversky_twin(logits, labels, *WI.TVERSKY[name], True)
    assert abs(loss - float(ref.detach())) < 1e-12 and float(np.abs(grad - lg.grad.numpy()).max()) < 1e-14
    kept = WI.tversky_twin(logits, labels, *WI.TVERSKY[name], False)[0]
    assert np.isfinite(kept) and kept != loss


def test_training_above_the_bound_is_refused_before_any_step():
    """One clear error at the start of train / train_scenes / evaluate; building the model is not refused."""
    from randlanet._hip import HipKernelError
    from randlanet.model import Model
    from randlanet.utils.losses import check_trainable_classes
    from randlanet.utils.modules import RandLANetSettings
    from randlanet.utils.trainer import TrainingSettings
    check_trainable_classes(256, "x")
    with pytest.raises(HipKernelError, match="n_classes=257 exceeds the 256 classes"):
        check_trainable_classes(257, "x")
    model = Model(RandLANetSettings(n_classes=300, n_points=128, n_neighbors=4, layer_sizes=[16, 32]), use_gpu=False)
    names = [f"c{i}" for i in range(300)]
    with pytest.raises(HipKernelError, match="Model.train: n_classes=300 exceeds the 256 classes"):
        model.train([], [], TrainingSettings(epochs=1, batch_size=2), class_names=names)
    with pytest.raises(HipKernelError, match="Model.evaluate: n_classes=300 exceeds the 256 classes"):
        model.evaluate([], names)


def test_class_weights_of_256_classes():
    from randlanet.utils.losses import check_class_weights, class_weights_from_counts
    counts = WI.inputs(256)[2]
    w = check_class_weights(class_weights_from_counts(counts), 256, 1)
    assert w.dtype == np.float32 and w.shape == (256,) and (w > 0).all()
