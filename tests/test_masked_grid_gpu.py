"""Grid subsampling of a partly labelled scan on the device against its host twin."""
import numpy as np
import pytest

from masked_inputs import partly_labelled_scene

pytestmark = pytest.mark.gpu


def test_device_grid_subsample_with_unlabelled_points_equals_the_host_twin():
    from randlanet.utils import grid as G
    xyz, feats, labels = partly_labelled_scene()
    want = G.grid_subsample_host(xyz, feats, labels, cell=0.1, n_classes=5, allow_unlabelled=True)
    got = G.grid_subsample(xyz, feats, labels, cell=0.1, n_classes=5, device="cuda", allow_unlabelled=True)
    assert (want.labels == -1).any() and (want.labels >= 0).any()
    for name in ("xyz", "features", "labels", "inverse", "count"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    with pytest.raises(ValueError, match="is outside"):
        G.grid_subsample(xyz, feats, labels, cell=0.1, n_classes=5, device="cuda")
