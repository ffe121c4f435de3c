"""Shared inputs and yardsticks of the outlier-removal tests (test_outliers_*): the seeded synthetic cases, an all-pairs
numpy yardstick that is independent of the package's K-NN and filter (it shares only boxes.fixed_sums, the definition of
the sum order), and the twin's result per case (computed once, never modified).  A case is (xyz (M, 3) float32, k,
std_ratio)."""
import numpy as np

import normals_inputs as ni

F32 = np.float32
N_SPIKES = 12
_cases, _twins, _yards = {}, {}, {}

CASES = ("surface_spikes_1", "surface_spikes_2", "surface_spikes_3",      # a noisy surface and 12 points floating off it
         "below_grid_k3", "below_grid_k63",     # 300 points, below the K-NN's grid threshold: the brute-force path
         "smallest",                            # M = k + 1: every point's neighbourhood is the whole cloud
         "coincident",                          # 50 copies of one point: m = mu = sigma = t = 0, every point kept by <=
         "duplicates",                          # duplicated points: ties and zero distances
         "chunk_1023", "chunk_1024", "chunk_1025",      # one chunk short of full, full, and a second chunk of one member
         "many_chunks")                         # 69 chunks: the second-level lanes 0 .. 4 take two turns
ALL_PAIRS = tuple(c for c in CASES if c != "many_chunks")     # the cases small enough for the all-pairs yardstick


def spikes(seed):
    """(xyz (1012, 3), is_spike (1012,) bool): normals_inputs' surface (noise 0.01) plus 12 points with x, y uniform in
    [-1, 1] and |z| uniform in [0.6, 1.5] (the surface stays inside |z| < 0.55), rows permuted."""
    rs = np.random.RandomState(seed)
    surf = ni._surface(rs, 1000)
    xy = rs.uniform(-1, 1, (N_SPIKES, 2))
    z = rs.uniform(0.6, 1.5, N_SPIKES) * rs.choice([-1.0, 1.0], N_SPIKES)
    xyz = np.concatenate([surf, np.concatenate([xy, z[:, None]], axis=1).astype(F32)])
    flag = np.arange(xyz.shape[0]) >= 1000
    perm = rs.permutation(xyz.shape[0])
    return np.ascontiguousarray(xyz[perm], dtype=F32), flag[perm]


def case(name):
    if name not in _cases:
        rs = np.random.RandomState(sum(map(ord, name)))
        if name.startswith("surface_spikes_"):
            c = (spikes(int(name[-1]))[0], 16, 2.0)
        elif name.startswith("below_grid_k"):
            c = (np.random.RandomState(77).uniform(-1, 1, (300, 3)).astype(F32), int(name.split("_k")[1]), 2.0)
        elif name == "smallest":
            c = (rs.uniform(-1, 1, (4, 3)).astype(F32), 3, 2.0)
        elif name == "coincident":
            c = (np.tile(np.array([[0.25, -1.5, 3.0]], F32), (50, 1)), 8, 1.0)
        elif name == "duplicates":
            c = (np.array(ni.cloud("duplicates")), 10, 2.0)
        elif name.startswith("chunk_"):
            c = (rs.uniform(-1, 1, (int(name.split("_")[1]), 3)).astype(F32), 8, 1.5)
        elif name == "many_chunks":
            c = (rs.uniform(0, 10, (70000, 3)).astype(F32), 8, 1.0)
        else:
            raise KeyError(name)
        c[0].setflags(write=False)
        _cases[name] = c
    return _cases[name]


def _frozen(res):
    for a in res[:4]:
        a.setflags(write=False)
    return res


def twin(name):
    """OutlierResult of the numpy twin for the case (computed once)."""
    if name not in _twins:
        from randlanet.utils.outliers import statistical_outliers_host
        _twins[name] = _frozen(statistical_outliers_host(*case(name)))
    return _twins[name]


def yardstick(name):
    """OutlierResult by all pairs: d2 = (dx*dx + dy*dy) + dz*dz with every operation rounded to float32, each row sorted, then
    the contract of utils/outliers.py written out once more; boxes.fixed_sums for the two sums (computed once)."""
    if name not in _yards:
        from randlanet.utils.boxes import fixed_sums
        from randlanet.utils.outliers import OutlierResult
        xyz, k, ratio = case(name)
        x = np.asarray(xyz, dtype=F32)
        M = x.shape[0]
        d = x[:, None, :] - x[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert d2.dtype == F32
        d2 = np.sort(d2, axis=1)[:, :k + 1].astype(np.float64)
        m = np.zeros(M, np.float64)
        for j in range(k + 1):
            m = m + np.sqrt(d2[:, j])
        m = m / np.float64(k)
        mu = fixed_sums(m[:, None], np.array([M]))[0, 0] / np.float64(M)
        sigma = np.sqrt(fixed_sums(((m - mu) * (m - mu))[:, None], np.array([M]))[0, 0] / np.float64(M - 1))
        t = mu + np.float64(ratio) * sigma
        keep = m <= t
        kept = np.flatnonzero(keep).astype(np.int64)
        slot = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
        _yards[name] = _frozen(OutlierResult(keep, kept, slot, m, np.float64(mu), np.float64(sigma), np.float64(t)))
    return _yards[name]


def bits(x):
    return np.asarray(x, dtype=np.float64).reshape(-1).view(np.uint64)


def assert_same(got, want, what=""):
    """Bit for bit: the float64 fields as uint64 views, the integer fields exactly, types and shapes included."""
    for f in ("mean", "std", "threshold"):
        assert bits(getattr(got, f))[0] == bits(getattr(want, f))[0], (what, f, getattr(got, f), getattr(want, f))
    g, w = got.mean_distance, want.mean_distance
    assert g.dtype == np.float64 and g.shape == w.shape, (what, g.dtype, g.shape)
    same = bits(g) == bits(w)
    assert same.all(), (what, "mean_distance", int((~same).sum()), g[~same][:3], w[~same][:3])
    for f, dt in (("keep", np.bool_), ("kept", np.int64), ("slot", np.int32)):
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == dt and g.shape == w.shape and np.array_equal(g, w), (what, f, g.dtype, g.shape, w.shape)
