"""Shared inputs and yardsticks of the normal-estimation tests (test_normals_*): the seeded synthetic cases, an all-pairs
numpy K-NN that is independent of the package, and the twin's result per case (computed once, never modified).  A case is
(xyz (M, 3) float32, k, viewpoint); every cloud comes with viewpoint None and with the origin."""
import numpy as np

F32 = np.float32
_clouds, _twins, _covs = {}, {}, {}

# cloud -> k
CLOUDS = {
    "surface_1000": 16,       # a noisy curved surface
    "noise_300_k3": 3,        # uniform noise below the K-NN's 512-point grid threshold: the brute-force path
    "noise_300_k64": 64,
    "three_points": 3,        # M == k
    "coincident": 16,         # 40 copies of one point plus noise points: neighbourhoods with tr == 0
    "line": 8,                # every neighbourhood on one line: two zero eigenvalues
    "plane": 12,              # on the exact plane z = const: normal exactly (0, 0, +-1), curvature exactly 0
    "duplicates": 10,         # duplicated points: K-NN ties broken by index
    "offset_1e3": 16,         # coordinates offset by 1e3: centring matters
}
RANDOM = ("surface_1000", "noise_300_k3", "noise_300_k64")        # the cases whose eigenvalue gaps were measured
CASES = [f"{c}-{v}" for c in CLOUDS for v in ("up", "origin")]


def _surface(rs, M, noise=0.01):
    u = rs.uniform(-1, 1, (M, 2))
    z = 0.3 * np.sin(2.0 * u[:, 0]) * np.cos(1.5 * u[:, 1]) + 0.2 * u[:, 0] * u[:, 1]
    return (np.stack([u[:, 0], u[:, 1], z], axis=1) + noise * rs.randn(M, 3)).astype(F32)


def cloud(name):
    if name not in _clouds:
        rs = np.random.RandomState(sum(map(ord, name.split("_k")[0])))       # (the two noise_300 cases share a cloud)
        if name == "surface_1000":
            xyz = _surface(rs, 1000) + np.array([0.5, -0.25, 2.0], F32)
        elif name.startswith("noise_300"):
            xyz = rs.uniform(-1, 1, (300, 3)).astype(F32)
        elif name == "three_points":
            xyz = np.array([[0.0, 0.0, 1.0], [1.0, 0.25, 1.5], [-0.5, 2.0, 0.75]], F32)
        elif name == "coincident":
            xyz = np.concatenate([np.tile(np.array([[0.25, -1.5, 3.0]], F32), (40, 1)),
                                  rs.uniform(-2, 2, (200, 3)).astype(F32) + np.array([0, 0, 3], F32)])
            xyz = xyz[rs.permutation(xyz.shape[0])]
        elif name == "line":
            t = rs.permutation(64).astype(F32) * F32(0.125)                  # exact in float32
            xyz = np.stack([t, F32(2) * t + F32(1), F32(-0.5) * t + F32(4)], axis=1).astype(F32)
        elif name == "plane":
            xyz = np.concatenate([rs.uniform(-1, 1, (400, 2)), np.full((400, 1), 1.75)], axis=1).astype(F32)
        elif name == "duplicates":
            base = rs.uniform(-1, 1, (90, 3)).astype(F32)
            xyz = np.concatenate([base, base, base[:31]])
            xyz = xyz[rs.permutation(xyz.shape[0])]
        elif name == "offset_1e3":
            xyz = _surface(rs, 700) + np.array([1000.0, -1000.0, 1000.0], F32)
        else:
            raise KeyError(name)
        xyz = np.ascontiguousarray(xyz, dtype=F32)
        xyz.setflags(write=False)
        _clouds[name] = xyz
    return _clouds[name]


def case(name):
    """(xyz, k, viewpoint) of a case name "<cloud>-up" or "<cloud>-origin"."""
    c, v = name.rsplit("-", 1)
    return cloud(c), CLOUDS[c], None if v == "up" else (0.0, 0.0, 0.0)


def twin(name):
    """NormalResult of the numpy twin for the case (computed once)."""
    if name not in _twins:
        from randlanet.utils.normals import estimate_normals_host
        xyz, k, vp = case(name)
        res = estimate_normals_host(xyz, k, vp)
        for a in res:
            a.setflags(write=False)
        _twins[name] = res
    return _twins[name]


def covariances(cname):
    """The twin's (M, 6) float64 covariances of a cloud (computed once)."""
    if cname not in _covs:
        from randlanet.utils.normals import covariances_host
        c = covariances_host(cloud(cname), CLOUDS[cname])
        c.setflags(write=False)
        _covs[cname] = c
    return _covs[cname]


def brute_knn(xyz, k):
    """(M, k) int64: all-pairs K-NN by the contract's metric - d2 = (dx*dx + dy*dy) + dz*dz, every operation rounded to
    float32 - ascending by (d2, index).  Independent of the package."""
    x = np.asarray(xyz, dtype=F32)
    d = x[:, None, :] - x[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == F32
    return np.argsort(d2, axis=1, kind="stable")[:, :k].astype(np.int64)


def full_matrix(C):
    """(Q, 3, 3) symmetric matrices of (Q, 6) entries (00, 01, 02, 11, 12, 22)."""
    A = np.empty((C.shape[0], 3, 3), np.float64)
    A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2] = (C[:, e] for e in range(6))
    A[:, 1, 0], A[:, 2, 0], A[:, 2, 1] = A[:, 0, 1], A[:, 0, 2], A[:, 1, 2]
    return A


def assert_same(got, want, what=""):
    """Bit for bit, the sign of a zero included."""
    for f in ("normals", "curvature"):
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == w.dtype == F32 and g.shape == w.shape, (what, f, g.dtype, g.shape, w.shape)
        same = g.view(np.uint32) == w.view(np.uint32)
        assert same.all(), (what, f, int((~same).sum()), g[~same][:3], w[~same][:3])
