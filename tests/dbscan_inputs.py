"""Shared inputs and yardstick of the density-rule tests (test_dbscan_*): the named cases - the smallest shapes at which each
part of DBSCAN's min_samples can go wrong -, the brute-force definition - all pairwise float32 d2 in the contract's operation
order, the support, the core graph by plain label propagation and the border rule by an explicit loop, independent of the
package - and the twin's result per case (computed once, never modified).

Geometry used throughout: r = 0.25 (exact in float32, like its square), cell edge c = r * 1.0625 = 17/64.  A "clump" is four
points on the x axis inside 0.1875 of each other: each has support 4, so all are core at min_samples = 4."""
import numpy as np

F32 = np.float32
R = 0.25
CELL = 17.0 / 64.0
_cache, _brutes, _twins = {}, {}, {}


def _clump(x0, sign):
    """Four points at x0, x0 + sign * (0.15625, 0.171875, 0.1875), y = z = 0 (multiples of 2^-6: exact): of a clump that starts
    0.125 or more from the origin only the first point lies within r of the origin."""
    return np.array([[x0 + sign * d, 0.0, 0.0] for d in (0.0, 0.15625, 0.171875, 0.1875)], F32)


def _lattice_blob(x0):
    """40 points: 4 x 5 x 2 with spacing 0.05 from (x0, 0, 0): every one has well over 4 neighbours within r."""
    g = np.stack(np.meshgrid(np.arange(4), np.arange(5), np.arange(2), indexing="ij"), axis=-1).reshape(-1, 3)
    return (g * 0.05 + np.array([x0, 0.0, 0.0])).astype(F32)


def _around(centre, offsets):
    """centre first, then centre + every non-zero combination of the offsets per axis."""
    out = [np.zeros(3)]
    for dz in offsets:
        for dy in offsets:
            for dx in offsets:
                if (dx, dy, dz) != (0.0, 0.0, 0.0):
                    out.append(np.array([dx, dy, dz]))
    return (np.asarray(centre, np.float64) + np.asarray(out)).astype(F32)


def _uniform(rs, M, side):
    """M points in a cube; labels 0 .. 3 of which 0 is ignored, and -1 for every 50th.  Per label (M / 4) / side^3 * 4.19 r^3
    is about 3 neighbours within r: supports around 4, so that core, border and noise points all occur at min_samples = 5."""
    xyz = rs.uniform(0, side, (M, 3)).astype(F32)
    lab = rs.randint(0, 4, M).astype(np.int64)
    lab[::50] = -1
    return xyz, lab


def _make(name):
    """(xyz (M, 3) float32, labels (M,) int64, keyword arguments of euclidean_clusters incl. radius and min_samples)"""
    base = name.rsplit("_ms", 1)[0]
    rs = np.random.RandomState(sum(map(ord, base)))
    kw = dict(radius=R, min_samples=int(name.rsplit("_ms", 1)[1]))
    order = None
    if base == "bridge":
        # blob A x in [0, 0.15]; the chain at y = 0.1, z = 0 starts 0.245 behind A's face - exactly one blob point, (0.15, 0.1,
        # 0), lies within r of it - and goes on in steps of 0.8 r; blob B begins 0.245 behind the chain's last point
        chain = np.array([[0.15 + 0.245 + 0.2 * k, 0.1, 0.0] for k in range(5)], F32)
        xyz = np.concatenate([_lattice_blob(0.0), chain, _lattice_blob(float(chain[-1, 0]) + 0.245)])
        lab = np.full(85, 1)
        order = rs.permutation(85)
    elif base in ("border_tie", "border_no_bridge"):
        # A = points 4 .. 7 on the left (scanned first: lower keys), B = points 0 .. 3 on the right, the border point last
        p = [0.0, 0.0, 0.0] if base == "border_tie" else [0.0, 0.0625, 0.0]
        xyz = np.concatenate([_clump(0.1875, 1), _clump(-0.1875, -1), np.array([p], F32)])
        lab = np.full(9, 1)
    elif base == "border_nearest":            # A's first point (index 4) at 0.125, B's (index 0) at 0.1875
        xyz = np.concatenate([_clump(0.1875, 1), _clump(-0.125, -1), np.array([[0.0, 0.0, 0.0]], F32)])
        lab = np.full(9, 1)
    elif base == "border_is_smallest_index":  # point 0 borders A (5 .. 8); B (1 .. 4) lies far away
        xyz = np.concatenate([np.array([[0.0, 0.0, 0.0]], F32), _clump(3.0, 1), _clump(-0.1875, -1)])
        lab = np.full(9, 1)
    elif base.startswith("border_counts_for_min_points"):
        # four cores, two border points (0, 0, 0) and (-0.1875, 0.2, 0), and a second clump of another label that is kept
        xyz = np.concatenate([_clump(-0.1875, -1), np.array([[0.0, 0.0, 0.0], [-0.1875, 0.2, 0.0]], F32), _clump(5.0, 1),
                              _clump(5.0, 1)])
        lab = np.array([1] * 6 + [2] * 8)
        kw["min_points"] = 6 if base.endswith("_6") else 7
    elif base == "other_labels_do_not_count":
        c = np.array([[1.0, 1.0, 1.0]], F32)
        near = (c + rs.uniform(-0.1, 0.1, (12, 3))).astype(F32)
        xyz = np.concatenate([c, near])
        lab = np.array([1] + [2] * 3 + [0] * 3 + [-1] * 3 + [1 + (1 << 32)] * 3, np.int64)
    elif base == "all_noise":
        xyz, lab = rs.uniform(0, 1, (50, 3)).astype(F32), np.full(50, 1)
    elif base == "single":
        xyz, lab = np.array([[1.5, -2.0, 0.25]], F32), np.array([3])
    elif base == "duplicates":                # k = 5 coincident points
        xyz, lab = np.repeat(np.array([[0.3, -0.7, 2.0]], F32), 5, axis=0), np.full(5, 2)
    elif base == "at_r":                      # exactly r apart along an axis (0.25 and its square are exact): counts
        xyz, lab = np.array([[-1.0, 2.0, 3.0], [-1.0, 2.25, 3.0]], F32), np.array([1, 1])
    elif base == "at_r_beyond":               # one float32 step further: does not
        xyz = np.array([[-1.0, 2.0, 3.0], [-1.0, np.nextafter(F32(2.25), F32(3)), 3.0]], F32)
        lab = np.array([1, 1])
    elif base in ("cells_27", "planar"):
        # the centre in the middle of cell (1, 1, 1) of a 3 x 3 x 3 grid, one neighbour in each of the 26 cells around it
        # (0.14 > c / 2 crosses into the next cell; 0.14 * sqrt(3) < r); min_samples = 27 needs every one of them
        xyz = _around([CELL * 10.5] * 3, (-0.14, 0.0, 0.14))
        if base == "planar":
            xyz[:, 2] = xyz[0, 2]
        lab = np.full(27, 1)
        order = rs.permutation(27)
    elif base == "corner":
        # the grid's first cell and its last one: a centre with its 7 neighbours in the cells after it, and another (label
        # 2) with them in the cells before it
        a = _around([CELL * 10.5] * 3, (0.0, 0.14))
        b = _around([CELL * 10.5 + 2.0] * 3, (0.0, -0.14))
        xyz, lab = np.concatenate([a, b]), np.repeat([1, 2], 8)
        order = rs.permutation(16)
    elif base == "uniform_4097":
        xyz, lab = _uniform(rs, 4097, 2.8)
    elif base == "uniform_20000":
        xyz, lab = _uniform(rs, 20000, 4.8)
    elif base in ("smooth_dense", "smooth_dense_curv"):
        # the floor z = 0 (normals +-z) and the wall x = 0 (normals +-x) as lattices of spacing 0.2 = 0.8 r: a point reaches
        # its 4 axis neighbours (the next distance is 0.283), the wall's first row being the floor's neighbour across the
        # crease.  The floor point (0, 0, 0) has support 4 - itself, two of the floor, one of the wall - of which 3 agree
        t = np.arange(6) * 0.2
        u, v = (a.reshape(-1) for a in np.meshgrid(t, t, indexing="ij"))
        floor = np.stack([u, v, np.zeros_like(u)], axis=1)
        wall = np.stack([np.zeros_like(u), v, u + 0.2], axis=1)
        xyz = np.concatenate([floor, wall]).astype(F32)
        nrm = np.concatenate([np.tile([0.0, 0.0, 1.0], (36, 1)), np.tile([1.0, 0.0, 0.0], (36, 1))]).astype(F32)
        nrm *= rs.choice([-1.0, 1.0], (72, 1)).astype(F32)             # whichever way a normal was turned
        lab = np.full(72, 1)
        order = rs.permutation(72)
        kw.update(normals=nrm[order], normal_angle=30.0)
        if base.endswith("_curv"):            # the points next to the crease take no part
            curv = np.where((xyz[:, 0] < 0.05) & (xyz[:, 2] < 0.25), 0.2, 0.01).astype(F32)
            kw.update(curvature=curv[order], max_curvature=0.1)
    else:
        raise KeyError(name)
    if order is not None:
        xyz, lab = xyz[order], np.asarray(lab)[order]
    if base in ("uniform_4097", "uniform_20000", "other_labels_do_not_count"):
        kw["ignore_classes"] = (0,)
    return np.ascontiguousarray(xyz, dtype=F32), np.asarray(lab, np.int64), kw


CASES = ("bridge_ms1", "bridge_ms4", "border_tie_ms4", "border_nearest_ms4", "border_no_bridge_ms4",
         "border_is_smallest_index_ms4", "border_counts_for_min_points_6_ms4", "border_counts_for_min_points_7_ms4",
         "other_labels_do_not_count_ms1", "other_labels_do_not_count_ms2", "all_noise_ms51", "single_ms1", "single_ms2",
         "duplicates_ms5", "duplicates_ms6", "at_r_ms2", "at_r_beyond_ms2", "cells_27_ms27", "planar_ms27", "corner_ms8",
         "uniform_4097_ms2", "uniform_4097_ms5", "uniform_20000_ms2", "uniform_20000_ms5", "smooth_dense_ms4",
         "smooth_dense_curv_ms4")


def case(name):
    """(xyz, labels, keywords) - made once, never modified."""
    if name not in _cache:
        _cache[name] = _make(name)
    return _cache[name]


def scores_of(name):
    """Per-point scores of a case, float32 in [0, 1)."""
    M = case(name)[0].shape[0]
    return np.random.RandomState(M).random_sample(M).astype(F32)


# ---------------------------------------------------------------------------------------------------- the definition
def brute_dense(xyz, labels, *, radius, min_samples, min_points=1, ignore_classes=(0,), scores=None, normals=None,
                normal_angle=None, curvature=None, max_curvature=None):
    """The contract restated in O(M^2): returns (result dict, support (M,), core (M,) bool, border (M,) bool)."""
    xyz = np.asarray(xyz).astype(F32)
    M = xyz.shape[0]
    r = F32(radius)
    r2 = r * r
    part = (labels >= 0) & ~np.isin(labels, np.asarray(ignore_classes, np.int64))
    if curvature is not None:
        part &= ~(np.asarray(curvature, F32) > F32(max_curvature))
    cos_t = F32(np.cos(np.float64(normal_angle) * np.pi / 180.0)) if normals is not None else None
    support = np.zeros(M, np.int64)
    ea, eb, ed = [], [], []                                  # the edges (both directions) under the rule asked for, with d2
    for i0 in range(0, M, 256):
        sl = slice(i0, i0 + 256)
        dx, dy, dz = (xyz[sl, None, k] - xyz[None, :, k] for k in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == F32
        near = (d2 <= r2) & (labels[sl, None] == labels[None, :]) & part[sl, None] & part[None, :]
        support[sl] = near.sum(axis=1)                       # the point itself included: d2 = 0
        a, b = np.nonzero(near)
        a = a + i0
        keep = a != b
        a, b, d = a[keep], b[keep], d2[a[keep] - i0, b[keep]]
        if normals is not None:
            na, nb = normals[a], normals[b]
            dot = (na[:, 0] * nb[:, 0] + na[:, 1] * nb[:, 1]) + na[:, 2] * nb[:, 2]
            assert dot.dtype == F32
            keep = np.abs(dot) >= cos_t
            a, b, d = a[keep], b[keep], d[keep]
        ea.append(a), eb.append(b), ed.append(d)
    ea, eb, ed = np.concatenate(ea), np.concatenate(eb), np.concatenate(ed)
    core = part & (support >= min_samples)
    # the core graph: every core point takes the smallest number among itself and the core points it has an edge to, until
    # nothing changes
    comp = np.arange(M)
    cc = core[ea] & core[eb]
    ca, cb = ea[cc], eb[cc]
    while True:
        new = comp.copy()
        np.minimum.at(new, ca, comp[cb])
        if np.array_equal(new, comp):
            break
        comp = new
    # the border rule, point by point
    border = np.zeros(M, bool)
    comp_of = np.where(core, comp, -1)
    cand = ~core[ea] & core[eb]
    by_point = {}
    for i, j, d in zip(ea[cand].tolist(), eb[cand].tolist(), ed[cand]):
        by_point.setdefault(i, []).append((d, j))
    for i, lst in by_point.items():
        best_d, best_j = lst[0]
        for d, j in lst[1:]:
            if d < best_d or (d == best_d and j < best_j):
                best_d, best_j = d, j
        border[i] = True
        comp_of[i] = comp[best_j]
    instance = np.full(M, -1, np.int32)
    out = dict(classes=[], count=[], centroid=[], lo=[], hi=[], score=[])
    for head in np.flatnonzero(core & (comp == np.arange(M))):                       # ascending smallest core point
        members = np.flatnonzero(comp_of == head)
        if members.size < min_points:
            continue
        instance[members] = len(out["count"])
        out["classes"].append(labels[head])
        out["count"].append(members.size)
        s, t = np.zeros(3, np.float64), np.float64(0)
        for m in members:                                                            # one by one, ascending index
            s = s + xyz[m].astype(np.float64)
            if scores is not None:
                t = t + np.float64(scores[m])
        out["centroid"].append((s / np.float64(members.size)).astype(F32))
        out["score"].append(F32(t / np.float64(members.size)))
        out["lo"].append(xyz[members].min(axis=0))
        out["hi"].append(xyz[members].max(axis=0))
    I = len(out["count"])
    res = dict(instance=instance, classes=np.asarray(out["classes"], np.int64).reshape(I),
               count=np.asarray(out["count"], np.int32).reshape(I), centroid=np.asarray(out["centroid"], F32).reshape(I, 3),
               lo=np.asarray(out["lo"], F32).reshape(I, 3), hi=np.asarray(out["hi"], F32).reshape(I, 3),
               score=np.asarray(out["score"], F32).reshape(I) if scores is not None else None)
    return res, support, core, border


def brute(name):
    """(result dict, support, core, border) of a case with scores_of(name) - computed once, shared, never modified."""
    if name not in _brutes:
        xyz, labels, kw = case(name)
        _brutes[name] = brute_dense(xyz, labels, scores=scores_of(name), **kw)
    return _brutes[name]


def twin(name):
    """ClusterResult of euclidean_clusters_host on the case with scores_of(name) - computed once, shared, never modified."""
    from randlanet.utils.cluster import euclidean_clusters_host
    if name not in _twins:
        xyz, labels, kw = case(name)
        _twins[name] = euclidean_clusters_host(xyz, labels, scores=scores_of(name), **kw)
    return _twins[name]
