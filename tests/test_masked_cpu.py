"""Host side of the masked loss mode (no GPU): the refusals of class weights, the authors' weight formula, the training
settings, and grid subsampling of partly labelled scans against a brute-force count per cell."""
import dataclasses

import numpy as np
import pytest

from masked_inputs import partly_labelled_scene
from randlanet.utils import grid as G
from randlanet.utils import losses as L
from randlanet.utils.trainer import TrainingSettings


@pytest.mark.parametrize("name", ["cross_entropy", "focal", "dice", "tversky", "focal_tversky"])
def test_class_weights_are_checked_on_the_host(name):
    for bad, what in (([1.0, -0.5, 1.0], ">= 0"), ([1.0, float("nan"), 1.0], "finite"), ([1.0, float("inf"), 1.0], "finite"),
                      ([0.0, 0.0, 0.0], "sum to zero"), ([[1.0, 1.0, 1.0]], "expected"), ([], "expected")):
        with pytest.raises(ValueError, match=what):
            L.get_loss(name, class_weights=bad)
    loss = L.get_loss(name, class_weights=[1.0, 2.0, 0.0])
    assert loss._ignore_unlabelled and loss._class_weights.tolist() == [1.0, 2.0, 0.0]
    assert not L.get_loss(name)._ignore_unlabelled and L.get_loss(name)._class_weights is None
    assert L.get_loss(name, ignore_unlabelled=True)._ignore_unlabelled


def test_constructors_take_and_check_the_weights():
    for make in (L.CrossEntropyLoss, L.FocalLoss, L.FocalTverskyLoss):
        with pytest.raises(ValueError, match=">= 0"):
            make(class_weights=[1.0, -1.0])
        with pytest.raises(ValueError, match="sum to zero"):
            make(class_weights=[0.0, 0.0])
        assert make(class_weights=[0.5, 1.5])._class_weights.tolist() == [0.5, 1.5]
    # wrong length: known where the class count is
    with pytest.raises(ValueError, match="expected 4 values"):
        L.check_class_weights([1.0, 1.0, 1.0], 4)


@pytest.mark.parametrize("name", ["dice", "tversky", "focal_tversky"])
def test_tversky_family_needs_weight_on_a_class_it_averages(name):
    with pytest.raises(ValueError, match="classes from 1 on"):
        L.get_loss(name, class_weights=[1.0, 0.0, 0.0])
    L.FocalTverskyLoss(neglect_background=False, class_weights=[1.0, 0.0, 0.0])      # class 0 is averaged there
    L.get_loss("cross_entropy", class_weights=[1.0, 0.0, 0.0])


def test_class_weights_from_counts_and_labels():
    np.testing.assert_array_equal(L.class_weights_from_counts([1, 3]), 1.0 / (np.array([0.25, 0.75]) + 0.02))
    a = np.array([0, 1, 1, 1, -1, 2, 255, -7])
    b = np.array([[1, 2], [5, 3]])
    np.testing.assert_array_equal(L.class_weights_from_labels([a], 2), L.class_weights_from_counts([1, 3]))
    np.testing.assert_array_equal(L.class_weights_from_labels([a, b], 3), L.class_weights_from_counts([1, 4, 2]))
    with pytest.raises(ValueError):
        L.class_weights_from_labels([np.array([-1, 7])], 3)


def test_training_settings_defaults():
    s = TrainingSettings()
    assert (s.epochs, s.batch_size, s.learning_rate, s.learning_rate_decay, s.loss_function, s.early_stopping,
            s.early_stopping_patience) == (150, 8, 1e-2, 0.9, "dice", True, 20)
    assert s.class_weights is None and s.ignore_unlabelled is False
    assert [f.name for f in dataclasses.fields(s)][:7] == ["epochs", "batch_size", "learning_rate", "learning_rate_decay",
                                                           "loss_function", "early_stopping", "early_stopping_patience"]


def test_grid_subsample_host_with_unlabelled_points():
    C, cell = 5, 0.1
    xyz, feats, labels = partly_labelled_scene()
    got = G.grid_subsample_host(xyz, feats, labels, cell=cell, n_classes=C, allow_unlabelled=True)
    V = got.count.size
    ok = (labels >= 0) & (labels < C)
    # brute force: a histogram per cell over the labelled points
    hist = np.zeros((V, C), np.int64)
    for i in np.flatnonzero(ok):
        hist[got.inverse[i], labels[i]] += 1
    n_lab = hist.sum(axis=1)
    n_unl = got.count - n_lab
    assert (n_lab == 0).any(), "no wholly unlabelled cell in the test input"
    assert ((n_unl > n_lab) & (n_lab > 0)).any(), "no cell with more unlabelled than labelled points"
    want = np.where(n_lab == 0, -1, np.argmax(hist, axis=1))
    np.testing.assert_array_equal(got.labels, want)
    assert got.labels.dtype == np.int64
    outvoted = (n_unl > n_lab) & (n_lab > 0)
    assert ((got.labels[outvoted] >= 0) & (got.labels[outvoted] < C)).all()
    # everything but the labels is what the same cloud gives with its labels clipped into range
    ref = G.grid_subsample_host(xyz, feats, np.clip(labels, 0, C - 1), cell=cell, n_classes=C)
    for name in ("xyz", "features", "inverse", "count"):
        a, b = getattr(got, name), getattr(ref, name)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    # in-range labels: the option changes nothing
    both = G.grid_subsample_host(xyz, feats, np.clip(labels, 0, C - 1), cell=cell, n_classes=C, allow_unlabelled=True)
    np.testing.assert_array_equal(both.labels, ref.labels)


def test_grid_subsample_refuses_unlabelled_points_by_default():
    xyz, feats, labels = partly_labelled_scene()
    first = int(np.flatnonzero((labels < 0) | (labels >= 5))[0])
    text = f"grid_subsample: label {int(labels[first])} of point {first} is outside \\[0, 5\\)"
    for kw in ({}, {"allow_unlabelled": False}):
        with pytest.raises(ValueError, match=text):
            G.grid_subsample_host(xyz, feats, labels, cell=0.1, n_classes=5, **kw)
        with pytest.raises(ValueError, match=text):
            G.grid_subsample(xyz, feats, labels, cell=0.1, n_classes=5, device="cpu", **kw)
