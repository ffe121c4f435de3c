"""Shared inputs and yardsticks of the smoothness-constrained clustering tests (test_smooth_cluster_*): the cases, the
brute-force definition - the all-pairs float32 matrix of cluster_inputs.brute_roots with the dot-product condition and the
curvature mask added, components by repeated min-propagation.  Nothing here imports the package; the twin's result per case
is in smooth_twin.py."""
import numpy as np

import cluster_inputs as ci

F32 = np.float32
_cache, _roots, _brutes = {}, {}, {}


def cos_of(angle):
    """The threshold of the contract: float32(cos(float64(angle) * pi / 180))."""
    return F32(np.cos(np.float64(angle) * np.pi / 180.0))


# 12 fixed unit directions: eleven 4.5 degrees apart on an arc of 45 degrees, where two agree within 40 degrees when they are
# at most eight steps apart and the ends of the arc only through the ones between them, and one at right angles to them all
_U = np.array([2.0, 1.0, 2.0]) / 3.0
_W = np.array([1.0, 2.0, -2.0]) / 3.0
DIRECTIONS = np.stack([np.cos(np.deg2rad(4.5 * k)) * _U + np.sin(np.deg2rad(4.5 * k)) * _W for k in range(11)]
                      + [np.cross(_U, _W)]).astype(F32)


def _plane(nx, ny, spacing=0.1):
    """An nx x ny lattice in the plane z = 0, float32."""
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return np.stack([i.ravel() * spacing, j.ravel() * spacing, np.zeros(nx * ny)], axis=1).astype(F32)


def _corner(rs, blend):
    """A floor patch z = 0 and a wall patch x = 0 that share an edge, 30 x 30 points each at spacing 0.1, in a random order.
    blend: the points within one spacing of the crease get the normal (1, 0, 1) / sqrt(2), which lies 45 degrees from both
    surfaces, as an estimated normal does there.  Returns (xyz, normals, near the crease (M,) bool)."""
    floor = _plane(30, 30)
    i, j = np.meshgrid(np.arange(30), np.arange(1, 31), indexing="ij")
    wall = np.stack([np.zeros(900), i.ravel() * 0.1, j.ravel() * 0.1], axis=1).astype(F32)
    xyz = np.concatenate([floor, wall])
    nrm = np.concatenate([np.tile([0.0, 0.0, 1.0], (900, 1)), np.tile([1.0, 0.0, 0.0], (900, 1))]).astype(F32)
    near = np.concatenate([floor[:, 0] < 0.15, wall[:, 2] < 0.15])
    if blend:
        nrm[near] = (np.array([1.0, 0.0, 1.0]) / np.sqrt(2.0)).astype(F32)
    order = rs.permutation(1800)
    return xyz[order], nrm[order], near[order]


def _make(name):
    """(xyz (M, 3) float32, labels (M,) int64, radius, keyword arguments of euclidean_clusters - normals and normal_angle
    among them)"""
    rs = np.random.RandomState(sum(map(ord, name.replace("_min5", ""))))
    if name.startswith("equal:"):             # every normal the same: the plain rule
        xyz, lab, r, kw = ci.case(name[6:])
        return xyz, lab, r, dict(kw, normals=np.tile(np.array([0, 0, 1], F32), (xyz.shape[0], 1)), normal_angle=10.0)
    if name.startswith("dense:") or name.startswith("curv:"):
        # the sizes from a CPU run of the brute force are asserted in test_smooth_cluster_cpu.py: components of many sizes,
        # the largest far above 100 points
        xyz, lab, r, kw = ci.case(name.split(":")[1])
        rs = np.random.RandomState(xyz.shape[0] + 7)
        kw = dict(kw, normals=DIRECTIONS[rs.randint(0, 12, xyz.shape[0])], normal_angle=40.0)
        if name.startswith("curv:"):
            kw.update(curvature=rs.uniform(0, 0.3, xyz.shape[0]).astype(F32), max_curvature=0.2)
            r = 2 * r                         # (at the case's own radius nearly every point stands alone)
        return xyz, lab, r, kw
    r = 0.15
    if name in ("corner", "corner_plain"):
        xyz, nrm, _ = _corner(rs, blend=False)
        kw = dict(normals=nrm, normal_angle=30.0) if name == "corner" else {}
    elif name in ("crease_bridges", "crease_cut"):      # at 80 degrees the blended normals of the crease join both surfaces
        xyz, nrm, near = _corner(rs, blend=True)
        kw = dict(normals=nrm, normal_angle=80.0)
        if name == "crease_cut":
            kw.update(curvature=np.where(near, 0.2, 0.0).astype(F32), max_curvature=0.1)
    elif name == "threshold":
        # points 0, 1: the dot product is 1 * cos_t + 0 * s + 0 * 0 = cos_t exactly: joined; points 2, 3: one float32 step
        # below: not joined
        c = cos_of(30.0)
        s = F32(np.sqrt(1.0 - np.float64(c) ** 2))
        xyz = np.array([[0, 0, 0], [0.1, 0, 0], [5, 0, 0], [5.1, 0, 0]], F32)
        nrm = np.array([[1, 0, 0], [c, s, 0], [1, 0, 0], [np.nextafter(c, F32(0)), s, 0]], F32)
        kw = dict(normals=nrm, normal_angle=30.0)
    elif name == "flipped":                   # one plane, half of the normals negated
        xyz = _plane(20, 20)
        nrm = np.tile(np.array([0, 0, 1], F32), (400, 1))
        nrm[rs.permutation(400)[:200]] *= F32(-1)
        kw = dict(normals=nrm, normal_angle=10.0)
    elif name == "zero_normals":              # a column of zero normals across a plane: two halves and 15 single points
        xyz = _plane(15, 15)
        nrm = np.tile(np.array([0, 0, 1], F32), (225, 1))
        nrm[np.abs(xyz[:, 0] - F32(0.7)) < 0.01] = 0
        kw = dict(normals=nrm, normal_angle=89.0)
    elif name in ("ring_10", "ring_3"):       # 72 points around a cylinder of radius 1, analytic normals 5 degrees apart
        t = np.deg2rad(5.0 * np.arange(72))
        order = rs.permutation(72)
        xyz = np.stack([np.cos(t), np.sin(t), np.full(72, 0.5)], axis=1).astype(F32)[order]
        nrm = np.stack([np.cos(t), np.sin(t), np.zeros(72)], axis=1).astype(F32)[order]
        r = 0.1                               # the chord to the next point is 0.0872, to the one after 0.174
        kw = dict(normals=nrm, normal_angle=10.0 if name == "ring_10" else 3.0)
    else:
        raise KeyError(name)
    lab = np.full(xyz.shape[0], 2, np.int64)
    return np.ascontiguousarray(xyz, dtype=F32), lab, r, kw


OWN = ("corner", "corner_plain", "crease_bridges", "crease_cut", "threshold", "flipped", "zero_normals", "ring_10", "ring_3")
DENSE = ("dense:one_cell_4096", "dense:uniform_20000", "dense:uniform_20000_min5", "curv:uniform_4097")
EQUAL = tuple("equal:" + n for n in ci.CASES)
CASES = OWN + DENSE + EQUAL


def case(name):
    """(xyz, labels, radius, keywords) - made once, never modified."""
    if name not in _cache:
        _cache[name] = _make(name)
    return _cache[name]


def scores_of(name):
    """Per-point scores of a case, float32 in [0, 1): those of cluster_inputs for a cloud of this size."""
    M = case(name)[0].shape[0]
    return np.random.RandomState(M).random_sample(M).astype(F32)


# ---------------------------------------------------------------------------------------------------- the definition
def brute_roots(xyz, labels, radius, ignore_classes=(0,), normals=None, normal_angle=None, curvature=None,
                max_curvature=None):
    """(root (M,), takes part (M,)): cluster_inputs.brute_roots with the smooth rule: a point with curvature >
    float32(max_curvature) takes no part, and an edge needs abs((nx_i*nx_j + ny_i*ny_j) + nz_i*nz_j) >= cos_t in float32."""
    xyz = np.asarray(xyz).astype(F32)
    M = xyz.shape[0]
    r = F32(radius)
    r2 = r * r
    part = (labels >= 0) & ~np.isin(labels, np.asarray(ignore_classes, np.int64))
    if curvature is not None:
        part = part & ~(np.asarray(curvature).astype(F32) > F32(max_curvature))
    if normals is not None:
        nrm, cos_t = np.asarray(normals).astype(F32), cos_of(normal_angle)
    rows, cols = [], []
    for i0 in range(0, M, 256):
        sl = slice(i0, i0 + 256)
        dx, dy, dz = (xyz[sl, None, k] - xyz[None, :, k] for k in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == F32
        adj = (d2 <= r2) & (labels[sl, None] == labels[None, :]) & part[sl, None] & part[None, :]
        if normals is not None:
            dot = (nrm[sl, None, 0] * nrm[None, :, 0] + nrm[sl, None, 1] * nrm[None, :, 1]) + nrm[sl, None, 2] * nrm[None, :, 2]
            assert dot.dtype == F32
            adj &= np.abs(dot) >= cos_t
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
    kw = dict(kw)
    M = xyz.shape[0]
    min_points = kw.pop("min_points", 1)
    cloud = name.replace("_min5", "")
    if cloud not in _roots:
        _roots[cloud] = brute_roots(xyz, labels, r, kw.pop("ignore_classes", (0,)), **kw)
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


assert_same = ci.assert_same
