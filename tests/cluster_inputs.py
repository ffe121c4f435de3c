"""Shared inputs and yardsticks of the Euclidean clustering tests (test_cluster_*): the cases, the brute-force definition -
the all-pairs float32 d2 matrix of the contract and components by repeated min-propagation, independent of the package - and
the twin's result per case (computed once, never modified)."""
import numpy as np

F32 = np.float32
_cache, _roots, _brutes, _twins = {}, {}, {}, {}


def _chain(rs, r, n, stretch=None):
    """n points spaced 0.9 r along the space diagonal, in a random order of the indices; stretch: one link of 1.01 r."""
    step = np.full(n, 0.9 * r)
    step[0] = 0.0
    if stretch is not None:
        step[stretch] = 1.01 * r
    t = np.cumsum(step) / np.sqrt(3.0)
    xyz = np.stack([t - 7.0, t + 3.0, t], axis=1).astype(F32)
    order = rs.permutation(n)
    return xyz[order], order


def _face_lattice(rs, M, spacing, half=7, offset=0.0):
    """Points exactly on cell faces: integer multiples of float32(spacing), computed in float32, around zero (then moved)."""
    return (rs.randint(-half, half + 1, (M, 3)).astype(F32) * F32(spacing) + F32(offset)).astype(F32)


def _blob(rs, centre, M, half):
    return (np.asarray(centre) + rs.uniform(-half, half, (M, 3))).astype(F32)


def _make(name):
    """(xyz (M, 3) float32, labels (M,) int64, radius, keyword arguments of euclidean_clusters)"""
    rs = np.random.RandomState(sum(map(ord, name.replace("_min5", ""))))          # (the two uniform_20000 cases share a cloud)
    kw = {}
    r = 0.25
    if name == "single":
        xyz, lab = np.array([[1.5, -2.0, 0.25]], F32), np.array([3])
    elif name == "pair_at_r":                 # exactly r apart along an axis: joined (0.25 and its square are exact)
        xyz, lab = np.array([[-1.0, 2.0, 3.0], [-1.0, 2.25, 3.0]], F32), np.array([1, 1])
    elif name == "pair_beyond_r":             # one float32 step further: not joined
        xyz = np.array([[-1.0, 2.0, 3.0], [-1.0, np.nextafter(F32(2.25), F32(3)), 3.0]], F32)
        lab = np.array([1, 1])
    elif name == "duplicates":
        base = rs.uniform(-1, 1, (40, 3)).astype(F32)
        xyz, lab = np.concatenate([base, base, base[:7]]), np.concatenate([np.arange(40) % 3 + 1] * 2 + [np.arange(7) % 3 + 1])
        r = 1e-3
    elif name == "all_ignored":
        xyz, lab = rs.uniform(0, 1, (300, 3)).astype(F32), rs.choice([0, -1, 7], 300)
        kw["ignore_classes"] = (0, 7)
    elif name == "chain_3000":
        xyz, _ = _chain(rs, r, 3000)
        lab = np.full(3000, 2)
    elif name == "chain_3000_cut":
        xyz, _ = _chain(rs, r, 3000, stretch=1777)
        lab = np.full(3000, 2)
    elif name in ("lattice_r", "lattice_0999r", "lattice_r_far", "lattice_0999r_far"):
        spacing = r if "_r" in name.replace("0999r", "") else 0.999 * r
        xyz = _face_lattice(rs, 3000, spacing, offset=8000.0 if name.endswith("_far") else 0.0)
        lab = rs.choice([1, 1, 1, 2], 3000)
    elif name == "touching_classes":          # two blobs of different classes that interpenetrate: never merged
        xyz = np.concatenate([_blob(rs, (0, 0, 0), 600, 0.5), _blob(rs, (0.9, 0, 0), 600, 0.5)])
        lab = np.repeat([1, 2], 600)
        r = 0.3
    elif name == "blobs_just_apart":          # same class, the gap r * (1 + 2^-10) wide
        r = 0.5
        a = _blob(rs, (-0.5, 0, 0), 500, 0.5)
        b = _blob(rs, (0.5, 0, 0), 500, 0.5)
        a[:, 0] = np.minimum(a[:, 0], 0.0)
        a[:20, 0] = 0.0                                           # points on both faces of the gap
        b[:, 0] = np.maximum(b[:, 0], 0.0) + r * (1 + 2.0 ** -10)
        b[:20, 0] = r * (1 + 2.0 ** -10)
        b[:20, 1:] = a[:20, 1:]                                   # straight across from each other
        xyz, lab = np.concatenate([a, b]).astype(F32), np.full(1000, 4)
    elif name == "one_cell_4096":             # everything inside one cell and within r of everything else
        r = 0.3
        xyz, lab = rs.uniform(0.32, 0.32 + 0.17, (4096, 3)).astype(F32), np.full(4096, 1)
    elif name in ("uniform_257", "uniform_4097"):
        M = int(name.split("_")[1])
        xyz, lab = rs.uniform(-3, 2, (M, 3)).astype(F32), rs.randint(0, 4, M)
        r = 0.45 if M == 257 else 0.2
    elif name in ("uniform_20000", "uniform_20000_min5"):
        # r fixed from a CPU run of the brute force: 1010 components at min_points = 1 (446 of two points or more, the
        # largest of 5361 points), 136 of them at min_points = 5
        xyz, lab = rs.uniform(-10, 10, (20000, 3)).astype(F32), rs.randint(0, 3, 20000)
        r = 1.0
        kw["ignore_classes"] = (1,)
        kw["min_points"] = 5 if name.endswith("min5") else 1
    elif name == "wide_pairs":                # about 56000 cells on two axes: the cell of a point is off by its roundings
        r = 1.0
        a = np.concatenate([rs.uniform(0, 59500, (1500, 2)), rs.uniform(0, 2, (1500, 1))], axis=1).astype(F32)
        u = rs.standard_normal((1500, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        b = a + (u * rs.choice([0.98, 0.999, 1.0, 1.001, 1.02], (1500, 1))).astype(F32)
        xyz, lab = np.concatenate([a, b]).astype(F32), np.full(3000, 1)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(xyz, dtype=F32), np.asarray(lab, np.int64), r, kw


CASES = ("single", "pair_at_r", "pair_beyond_r", "duplicates", "all_ignored", "chain_3000", "chain_3000_cut", "lattice_r",
         "lattice_0999r", "lattice_r_far", "lattice_0999r_far", "touching_classes", "blobs_just_apart", "one_cell_4096",
         "uniform_257", "uniform_4097", "uniform_20000", "uniform_20000_min5", "wide_pairs")


def case(name):
    """(xyz, labels, radius, keywords) - made once, never modified."""
    if name not in _cache:
        _cache[name] = _make(name)
    return _cache[name]


def scores_of(name):
    """Per-point scores of a case, float32 in [0, 1)."""
    M = case(name)[0].shape[0]
    return np.random.RandomState(M).random_sample(M).astype(F32)


# ---------------------------------------------------------------------------------------------------- the definition
def brute_roots(xyz, labels, radius, ignore_classes=(0,)):
    """(root (M,), takes part (M,)): the smallest point index of every point's component, from the all-pairs float32 matrix
    d2 = (dx*dx + dy*dy) + dz*dz <= r*r (built in blocks of rows) and min-propagation over it until nothing changes."""
    xyz = np.asarray(xyz).astype(F32)
    M = xyz.shape[0]
    r = F32(radius)
    r2 = r * r
    part = (labels >= 0) & ~np.isin(labels, np.asarray(ignore_classes, np.int64))
    rows, cols = [], []
    for i0 in range(0, M, 256):
        sl = slice(i0, i0 + 256)
        dx, dy, dz = (xyz[sl, None, k] - xyz[None, :, k] for k in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == F32
        adj = (d2 <= r2) & (labels[sl, None] == labels[None, :]) & part[sl, None] & part[None, :]
        adj[np.arange(adj.shape[0]), np.arange(i0, i0 + adj.shape[0])] = True        # every point reaches itself
        a, b = np.nonzero(adj)
        rows.append(a + i0)
        cols.append(b)
    a, b = np.concatenate(rows), np.concatenate(cols)
    first = np.flatnonzero(np.concatenate(([True], a[1:] != a[:-1])))                # a is sorted: the rows' first entries
    lab = np.arange(M)
    while True:
        new = np.minimum.reduceat(lab[b], first)
        if np.array_equal(new, lab):
            return lab, part
        lab = new


def brute(name):
    """The expected ClusterResult fields of a case as a dict, from brute_roots and the contract's rules restated."""
    if name in _brutes:
        return _brutes[name]
    xyz, labels, r, kw = case(name)
    M = xyz.shape[0]
    min_points = kw.get("min_points", 1)
    cloud = name.replace("_min5", "")
    if cloud not in _roots:
        _roots[cloud] = brute_roots(xyz, labels, r, kw.get("ignore_classes", (0,)))
    root, part = _roots[cloud]
    instance = np.full(M, -1, np.int32)
    out = dict(classes=[], count=[], centroid=[], lo=[], hi=[], score=[])
    sc = scores_of(name)
    for head in np.flatnonzero(part & (root == np.arange(M))):                      # ascending smallest member
        members = np.flatnonzero(part & (root == head))
        if members.size < min_points:
            continue
        instance[members] = len(out["count"])
        out["classes"].append(labels[head])
        out["count"].append(members.size)
        s, t = np.zeros(3, np.float64), np.float64(0)
        for m in members:                                                            # one by one, ascending index
            s = s + xyz[m].astype(np.float64)
            t = t + np.float64(sc[m])
        out["centroid"].append((s / np.float64(members.size)).astype(F32))
        out["score"].append(F32(t / np.float64(members.size)))
        out["lo"].append(xyz[members].min(axis=0))
        out["hi"].append(xyz[members].max(axis=0))
    I = len(out["count"])
    res = dict(instance=instance, classes=np.asarray(out["classes"], np.int64).reshape(I),
               count=np.asarray(out["count"], np.int32).reshape(I), centroid=np.asarray(out["centroid"], F32).reshape(I, 3),
               lo=np.asarray(out["lo"], F32).reshape(I, 3), hi=np.asarray(out["hi"], F32).reshape(I, 3),
               score=np.asarray(out["score"], F32).reshape(I))
    _brutes[name] = res
    return res


def twin(name):
    """ClusterResult of euclidean_clusters_host on the case with scores_of(name) - computed once, shared, never modified."""
    from randlanet.utils.cluster import euclidean_clusters_host
    if name not in _twins:
        xyz, labels, r, kw = case(name)
        _twins[name] = euclidean_clusters_host(xyz, labels, radius=r, scores=scores_of(name), **kw)
    return _twins[name]


def assert_same(res, ref, what=""):
    """Every array of a ClusterResult (or the dict of brute) equal: dtype, shape and every entry."""
    for f in ("instance", "classes", "count", "centroid", "lo", "hi", "score"):
        a = getattr(res, f)
        b = ref[f] if isinstance(ref, dict) else getattr(ref, f)
        if b is None:
            assert a is None, f"{what} {f}"
            continue
        assert a is not None and a.dtype == b.dtype and a.shape == b.shape, (what, f, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), f"{what} {f}: {int((a != b).sum())} entries differ"
