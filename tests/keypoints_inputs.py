"""Shared inputs and yardsticks of the keypoint tests (test_keypoints_*): the cases, the brute-force definition - the
all-pairs float32 d2 of the contract, support, live and peaks straight from their definitions, the weighted mean taken in
ascending INDEX order, independent of the package - and the twin's result per case (computed once, never modified)."""
import numpy as np

F32 = np.float32
FIELDS = ("index", "classes", "position", "score", "mean_score", "count")
DTYPES = dict(index=np.int64, classes=np.int64, position=F32, score=F32, mean_score=F32, count=np.int32)
_cache, _brutes, _twins = {}, {}, {}


def _sixteenths(rs, M, lo=0, hi=16):
    return (rs.randint(lo, hi + 1, M) / 16.0).astype(F32)


def _face_lattice(rs, M, spacing, half=7, offset=0.0):
    """Points exactly on cell faces: integer multiples of float32(spacing), computed in float32, around zero (then moved)."""
    return (rs.randint(-half, half + 1, (M, 3)).astype(F32) * F32(spacing) + F32(offset)).astype(F32)


def _neighbour_cells_26():
    """26 pairs, three cells apart along x: the weaker point 0.4 cell edges from the centre of its cell towards one of the 26
    cells around it, the stronger one 0.6 edges, hence inside that cell and 0.2 * |d| edges < 0.37 r away.  r = 0.25 makes
    the cell edge 17/64 exact, and a pair with d = -1 on every axis puts the grid's origin at 0."""
    r = 0.25
    c = np.float64(F32(r) * F32(1.0625))
    xyz, want = [], []
    ds = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]
    for k, (dz, dy, dx) in enumerate(ds):
        centre = (np.array([3 * k + 1, 1, 1]) + 0.5) * c
        d = np.array([dx, dy, dz], np.float64)
        xyz += [centre + 0.4 * c * d, centre + 0.6 * c * d]
    xyz = np.asarray(xyz).astype(F32)
    cell = np.floor(xyz.astype(np.float64) / c).astype(np.int64)
    assert cell.min() == 0 and np.array_equal(cell[1::2] - cell[0::2], np.array([(dx, dy, dz) for dz, dy, dx in ds]))
    return xyz, np.ones(52, np.int64), np.tile(np.array([0.5, 0.75], F32), 26), r


def _make(name):
    """(xyz (M, 3) float32, labels (M,) int64, scores (M,) float32, radius, keyword arguments of confidence_peaks)"""
    rs = np.random.RandomState(sum(map(ord, name)))
    kw = {}
    r = 0.25
    if name == "single":
        xyz, lab, sc = np.array([[1.5, -2.0, 0.25]], F32), np.array([3]), np.array([0.75], F32)
    elif name in ("pair_at_r", "equal_scores_pair"):      # exactly r apart along an axis (0.25 and its square are exact)
        xyz, lab = np.array([[-1.0, 2.0, 3.0], [-1.0, 2.25, 3.0]], F32), np.array([1, 1])
        sc = np.array([0.5, 0.75] if name == "pair_at_r" else [0.625, 0.625], F32)
    elif name == "pair_beyond_r":             # one float32 step further
        xyz = np.array([[-1.0, 2.0, 3.0], [-1.0, np.nextafter(F32(2.25), F32(3)), 3.0]], F32)
        lab, sc = np.array([1, 1]), np.array([0.5, 0.75], F32)
    elif name in ("plateau_4096", "plateau_4097"):        # everything inside one cell and within r of everything else
        M = int(name.split("_")[1])
        r = 0.3
        xyz, lab, sc = rs.uniform(0.32, 0.32 + 0.17, (M, 3)).astype(F32), np.full(M, 1), np.full(M, 0.5, F32)
    elif name == "duplicates":
        base, s = rs.uniform(-1, 1, (40, 3)).astype(F32), _sixteenths(rs, 40, 4)
        xyz, sc = np.concatenate([base, base, base[:7]]), np.concatenate([s, s, s[:7]])
        lab = np.concatenate([np.arange(40) % 3 + 1] * 2 + [np.arange(7) % 3 + 1])
        r = 1e-3
    elif name == "neighbour_cells_26":
        xyz, lab, sc, r = _neighbour_cells_26()
    elif name in ("lattice_r", "lattice_0999r", "lattice_r_far", "lattice_0999r_far"):
        spacing = r if "_r" in name.replace("0999r", "") else 0.999 * r
        xyz = _face_lattice(rs, 3000, spacing, offset=8000.0 if name.endswith("_far") else 0.0)
        lab, sc = rs.choice([1, 1, 1, 2], 3000), _sixteenths(rs, 3000)
    elif name == "flat":                      # one layer of cells in z
        xyz = np.concatenate([rs.uniform(-3, 2, (2000, 2)), np.full((2000, 1), 1.0)], axis=1).astype(F32)
        lab, sc, r = rs.randint(0, 4, 2000), _sixteenths(rs, 2000), 0.2
    elif name == "corner":                    # a blob in every corner cell of the grid
        corners = np.array([(x, y, z) for x in (-2, 2) for y in (-2, 2) for z in (-2, 2)], np.float64)
        xyz = (np.repeat(corners, 30, axis=0) + rs.uniform(-0.1, 0.1, (240, 3))).astype(F32)
        lab, sc = rs.randint(1, 4, 240), _sixteenths(rs, 240)
    elif name == "touching_classes":          # two blobs of different classes that interpenetrate
        xyz = np.concatenate([rs.uniform(-0.5, 0.5, (600, 3)), rs.uniform(-0.5, 0.5, (600, 3)) + (0.9, 0, 0)]).astype(F32)
        lab, sc, r = np.repeat([1, 2], 600), _sixteenths(rs, 1200), 0.3
    elif name == "wide_labels":               # labels that agree in their low 32 bits only
        xyz = rs.uniform(-1, 1, (1500, 3)).astype(F32)
        lab, sc, r = rs.choice([1, 1 + (1 << 32), 2, 2 + (1 << 32), 2 + (1 << 40)], 1500), _sixteenths(rs, 1500), 0.2
    elif name == "lone_outlier":
        # point 0 is the blob's strongest (0.75) and its nearest to the outlier, point 40 (score 1.0, 0.24 away); every other
        # blob point is 0.29 or more from the outlier, which so has two participating points within r: not live at 3
        blob = np.concatenate([rs.uniform(0.05, 0.1, (39, 1)), rs.uniform(-0.02, 0.02, (39, 2))], axis=1)
        xyz = np.concatenate([[[0.0, 0.0, 0.0]], blob, [[-0.24, 0.0, 0.0]]]).astype(F32)
        lab, sc = np.full(41, 1), np.concatenate([[0.75], _sixteenths(rs, 39, 4, 8), [1.0]]).astype(F32)
        kw["min_points"] = 3
    elif name == "nothing":                   # ignored, unlabelled, or below min_score
        xyz, lab = rs.uniform(0, 1, (300, 3)).astype(F32), rs.choice([0, -1, 7, 1], 300)
        sc = np.where(lab == 1, _sixteenths(rs, 300, 0, 7), _sixteenths(rs, 300))
        kw.update(ignore_classes=(0, 7), min_score=0.5)
    elif name == "zero_scores":
        xyz, lab, sc, r = rs.uniform(-1, 1, (500, 3)).astype(F32), rs.randint(0, 4, 500), np.zeros(500, F32), 0.3
    elif name in ("uniform_2049", "uniform_4097"):
        M = int(name.split("_")[1])
        xyz, lab, sc, r = rs.uniform(-3, 2, (M, 3)).astype(F32), rs.randint(0, 4, M), _sixteenths(rs, M), 0.45
        kw.update(min_score=0.25, min_points=2 if M == 4097 else 1)
    elif name == "uniform_20000":
        xyz, lab, sc, r = rs.uniform(-10, 10, (20000, 3)).astype(F32), rs.randint(0, 4, 20000), _sixteenths(rs, 20000), 1.0
        kw.update(min_score=0.25, min_points=3, ignore_classes=(1,))
    else:
        raise KeyError(name)
    return np.ascontiguousarray(xyz, dtype=F32), np.asarray(lab, np.int64), np.ascontiguousarray(sc, dtype=F32), r, kw


CASES = ("single", "pair_at_r", "pair_beyond_r", "equal_scores_pair", "plateau_4096", "plateau_4097", "duplicates",
         "neighbour_cells_26", "lattice_r", "lattice_0999r", "lattice_r_far", "lattice_0999r_far", "flat", "corner",
         "touching_classes", "wide_labels", "lone_outlier", "nothing", "zero_scores", "uniform_2049", "uniform_4097",
         "uniform_20000")


def case(name):
    """(xyz, labels, scores, radius, keywords) - made once, never modified."""
    if name not in _cache:
        _cache[name] = _make(name)
    return _cache[name]


def too_fine():
    """The pair of test_cluster_gpu.py that is refused at radius 1.0 and accepted at 1.1, with labels and scores."""
    return np.array([[0, 0, 0], [0, 70000, 0], [1, 2, 3]], F32), np.ones(3, np.int64), np.array([0.5, 0.75, 1.0], F32)


# ---------------------------------------------------------------------------------------------------- the definition
def _near_rows(xyz, labels, part, r2, rows):
    """(len(rows), M) bool: part(j) and near(i, j) for i in rows, from the float32 d2 = (dx*dx + dy*dy) + dz*dz <= r2."""
    dx, dy, dz = (xyz[rows, None, k] - xyz[None, :, k] for k in range(3))
    d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == F32
    return (d2 <= r2) & (labels[rows, None] == labels[None, :]) & part[None, :]


def brute_peaks(xyz, labels, scores, radius, min_score=0.0, min_points=1, ignore_classes=(0,)):
    """(peaks ascending, live (M,) bool, part (M,) bool) straight from the definition, in blocks of rows."""
    M = xyz.shape[0]
    r = F32(radius)
    r2 = r * r
    part = (labels >= 0) & ~np.isin(labels, np.asarray(ignore_classes, np.int64)) & (scores >= F32(min_score))
    P = np.flatnonzero(part)
    support = np.zeros(M, np.int64)
    for i0 in range(0, P.size, 256):
        rows = P[i0:i0 + 256]
        support[rows] = _near_rows(xyz, labels, part, r2, rows).sum(axis=1)
    live = part & (support >= min_points)
    L = np.flatnonzero(live)
    peaks = []
    for i0 in range(0, L.size, 256):
        rows = L[i0:i0 + 256]
        near = _near_rows(xyz, labels, live, r2, rows)
        beats = (scores[None, :] > scores[rows, None]) | ((scores[None, :] == scores[rows, None]) &
                                                          (np.arange(M)[None, :] < rows[:, None]))
        peaks += rows[~(near & beats).any(axis=1)].tolist()
    return np.asarray(peaks, np.int64), live, part


def brute(name):
    """The expected KeypointResult fields of a case as a dict, from brute_peaks and the contract's rules restated; the sums
    run over the members in ascending point index (the twin's run in sorted-cell order: the positions may differ by the
    bound of test_keypoints_cpu.py)."""
    if name in _brutes:
        return _brutes[name]
    xyz, labels, scores, r, kw = case(name)
    peaks, live, _ = brute_peaks(xyz, labels, scores, r, **kw)
    r32 = F32(r)
    out = dict(position=[], mean_score=[], count=[])
    for p in peaks.tolist():
        members = np.flatnonzero(_near_rows(xyz, labels, live, r32 * r32, np.array([p]))[0])
        W, S = 0.0, [0.0, 0.0, 0.0]
        for j in members.tolist():                                                   # one by one, ascending index
            s = float(scores[j])
            W = W + s
            for a in range(3):
                S[a] = S[a] + s * (float(xyz[j, a]) - float(xyz[p, a]))
        out["position"].append([F32(float(xyz[p, a]) + S[a] / W) if W != 0.0 else xyz[p, a] for a in range(3)])
        out["mean_score"].append(F32(W / float(members.size)))
        out["count"].append(members.size)
    Kn = peaks.size
    res = dict(index=peaks, classes=labels[peaks], position=np.asarray(out["position"], F32).reshape(Kn, 3),
               score=scores[peaks], mean_score=np.asarray(out["mean_score"], F32).reshape(Kn),
               count=np.asarray(out["count"], np.int32).reshape(Kn))
    _brutes[name] = res
    return res


def twin(name):
    """KeypointResult of confidence_peaks_host on the case - computed once, shared, never modified."""
    from randlanet.utils.keypoints import confidence_peaks_host
    if name not in _twins:
        xyz, labels, scores, r, kw = case(name)
        _twins[name] = confidence_peaks_host(xyz, labels, scores, radius=r, **kw)
    return _twins[name]


def assert_same(res, ref, what=""):
    """Every array of a KeypointResult (or the dict of brute) equal: dtype, shape and every entry."""
    for f in FIELDS:
        a = getattr(res, f)
        b = ref[f] if isinstance(ref, dict) else getattr(ref, f)
        assert a.dtype == b.dtype == DTYPES[f] and a.shape == b.shape, (what, f, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), f"{what} {f}: {int((a != b).sum())} entries differ"
