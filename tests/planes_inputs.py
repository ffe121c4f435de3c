"""Shared inputs and yardsticks of the plane-segmentation tests (test_planes_*): the seeded synthetic cases, a yardstick that
is independent of the package's fit (it shares only boxes.fixed_sums, the definition of the sum order), and the twin's
result per case (computed once, never modified).  A case is (xyz (M, 3) float32, keywords of fit_plane_host); `room` is the
one case of segment_planes and has its own accessors."""
import numpy as np

F32 = np.float32
NORMAL = np.array([0.2, -0.3, 1.0]) / np.linalg.norm([0.2, -0.3, 1.0])     # the table's true normal, tilted 19.8 degrees
OFFSET = 0.4                                                               # NORMAL . p = OFFSET on the table
_cases, _twins, _yards = {}, {}, {}

CASES = ("table_1", "table_2", "table_3",       # 1000 points of a noisy plane and 500 of clutter above it, T = 256
         "chunk_1023", "chunk_1024", "chunk_1025",      # table_1 cut at the edges of the compaction's chunk
         "edge_shell",                          # 2000 points within 4e-6 of |s| = threshold: contraction changes the counts
         "lattice",                             # every distance exact: the +-0.25 layers are in by <=
         "ties",                                # equal counts: the lower index wins
         "degenerate",                          # repeated index, collinear and coincident points: NaN rows
         "one_point",                           # 50 copies of one point: no plane
         "smallest",                            # M = 3, T = 1
         "t_65",                                # T no multiple of 64
         "axis_10", "axis_30",                  # table_1 with the axis rule
         "many_chunks")                         # 70 000 points: 274 chunks of the count table
SCALAR = ("lattice", "ties", "degenerate", "one_point", "smallest")    # small enough for the all-scalar yardstick


def table(seed, n_plane=1000, n_clutter=500, permute=True):
    """(xyz float64, on_plane bool): n_plane points of the plane NORMAL . p = OFFSET with in-plane coordinates uniform in
    [-1, 1]^2 and Gaussian noise 0.004 along the normal, n_clutter points uniform in [-1, 1]^2 x [0.45, 1.2]."""
    rs = np.random.RandomState(seed)
    a = np.cross(NORMAL, [1.0, 0.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(NORMAL, a)
    uv = rs.uniform(-1, 1, (n_plane, 2))
    plane = uv[:, :1] * a + uv[:, 1:] * b + OFFSET * NORMAL + rs.normal(0, 0.004, (n_plane, 1)) * NORMAL
    clutter = np.concatenate([rs.uniform(-1, 1, (n_clutter, 2)), rs.uniform(0.45, 1.2, (n_clutter, 1))], axis=1)
    xyz = np.concatenate([plane, clutter])
    flag = np.arange(xyz.shape[0]) < n_plane
    if permute:
        perm = rs.permutation(xyz.shape[0])
        xyz, flag = xyz[perm], flag[perm]
    return xyz, flag


def lattice():
    """320 points on multiples of 0.25: x, y in 0 .. 1.75, z in -0.5 .. 0.5; index = (zi * 8 + yi) * 8 + xi."""
    z, y, x = np.meshgrid(np.arange(-2, 3), np.arange(8), np.arange(8), indexing="ij")
    return (np.stack((x, y, z), axis=-1).reshape(-1, 3) * 0.25).astype(F32)


def _at(xi, yi, zi):
    return ((zi + 2) * 8 + yi) * 8 + xi


def _corner(xi, yi, zi):
    """An axis-aligned triple of the lattice in the layer zi: its plane is exactly z = 0.25 * zi."""
    return [_at(xi, yi, zi), _at(xi + 1, yi, zi), _at(xi, yi + 1, zi)]


def edge_shell():
    """The table (600 + 100 points) shifted by (7, -5, 3), rows 0, 1, 2 three of its plane points far apart; then 2000 points
    projected in float64 onto the plane of the triple (0, 1, 2) and moved along its normal by +-0.01 + uniform(-4e-6, 4e-6)."""
    rs = np.random.RandomState(404)
    xyz, flag = table(9, 600, 100, permute=False)
    xyz = xyz + np.array([7.0, -5.0, 3.0])
    rel = xyz[:600] - xyz[:600].mean(axis=0)
    far = [int(np.argmax(rel @ v)) for v in (rel[0], -rel[0], np.cross(NORMAL, rel[0]))]
    assert len(set(far)) == 3
    order = far + [i for i in range(700) if i not in far]
    base = xyz[order].astype(F32)
    n, d = (np.float64(v) for v in (_hypothesis(base, (0, 1, 2))[:3], _hypothesis(base, (0, 1, 2))[3]))
    q = base[rs.randint(0, 600, 2000)].astype(np.float64) + rs.uniform(-0.3, 0.3, (2000, 3))
    q = q - ((q @ n) + d)[:, None] * n
    q = q + ((rs.choice([-0.01, 0.01], 2000) + rs.uniform(-4e-6, 4e-6, 2000))[:, None]) * n
    cloud = np.concatenate([base, q.astype(F32)])
    tri = np.concatenate([[[0, 1, 2]], np.random.default_rng(5).integers(0, cloud.shape[0], (63, 3))]).astype(np.int64)
    return cloud, tri


def case(name):
    if name not in _cases:
        kw = dict(threshold=0.01, iterations=256, seed=0)
        if name.startswith("table_"):
            xyz, kw["seed"] = table(int(name[-1]))[0], int(name[-1])
        elif name.startswith("chunk_"):
            xyz, kw["seed"] = table(1)[0][:int(name.split("_")[1])], 1
        elif name == "edge_shell":
            xyz, tri = edge_shell()
            kw = dict(threshold=0.01, triples=tri)
        elif name == "lattice":
            xyz = lattice()
            kw = dict(threshold=0.25, triples=np.array([_corner(0, 0, 0), _corner(3, 2, 0), _corner(6, 6, 0), _corner(1, 5, 0)]))
        elif name == "ties":        # x = 0 (80 points), then z = 0.25 twice by the same triple and once by a disjoint one
            xyz = lattice()
            kw = dict(threshold=0.25, triples=np.array([[_at(0, 0, 0), _at(0, 1, 0), _at(0, 0, 1)], _corner(0, 0, 1),
                                                        _corner(0, 0, 1), _corner(4, 4, 1)]))
        elif name == "degenerate":
            xyz = np.random.RandomState(3).uniform(-1, 1, (40, 3))
            xyz[:3] = [[0, 0, 0], [0.5, 0.5, 0.5], [1, 1, 1]]          # collinear, exactly
            xyz[4] = xyz[3]                                             # coincident
            kw = dict(threshold=0.05, triples=np.array([[5, 5, 7], [0, 1, 2], [3, 4, 9], [10, 11, 12], [6, 6, 6]]))
        elif name == "one_point":
            xyz = np.tile(np.array([[0.25, -1.5, 3.0]]), (50, 1))
            kw = dict(threshold=0.01, iterations=16, seed=0)
        elif name == "smallest":
            xyz = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.25], [0.0, 1.0, -0.5]])
            kw = dict(threshold=0.01, triples=np.array([[0, 1, 2]]))
        elif name == "t_65":
            xyz, kw = table(1)[0], dict(threshold=0.01, iterations=65, seed=65)
        elif name.startswith("axis_"):
            xyz, kw = table(1)[0], dict(threshold=0.01, iterations=256, seed=1, axis=(0, 0, 1), max_angle=int(name[5:]))
        elif name == "many_chunks":
            rs = np.random.RandomState(70)
            xyz = np.concatenate([rs.uniform(0, 10, (50000, 3)),
                                  np.concatenate([rs.uniform(0, 10, (20000, 2)), rs.normal(4.0, 0.01, (20000, 1))], axis=1)])
            xyz, kw = xyz[rs.permutation(70000)], dict(threshold=0.03, iterations=64, seed=2)
        else:
            raise KeyError(name)
        xyz = np.ascontiguousarray(xyz, dtype=F32)
        xyz.setflags(write=False)
        _cases[name] = (xyz, kw)
    return _cases[name]


def _frozen(res):
    for a in res:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


def twin(name):
    """PlaneFit of the numpy twin for the case (computed once)."""
    if name not in _twins:
        from randlanet.utils.planes import fit_plane_host
        xyz, kw = case(name)
        _twins[name] = _frozen(fit_plane_host(xyz, **kw))
    return _twins[name]


# ------------------------------------------------------------------------------------------------------------- room
ROOM = dict(threshold=0.01, max_planes=4, min_points=500, iterations=512, seed=0)


def room():
    """(xyz (7500, 3) float32, surface (7500,) int: 0 floor, 1 the wall x ~ 0, 2 the wall y ~ 0, 3 clutter off all three)."""
    if "room" not in _cases:
        rs = np.random.RandomState(12)
        floor = np.stack((rs.uniform(0, 4, 3000), rs.uniform(0, 3, 3000), rs.normal(0, 0.003, 3000)), axis=1)
        wall_x = np.stack((rs.normal(0, 0.003, 1500), rs.uniform(0, 3, 1500), rs.uniform(0, 2.5, 1500)), axis=1)
        wall_y = np.stack((rs.uniform(0, 4, 1500), rs.normal(0, 0.003, 1500), rs.uniform(0, 2.5, 1500)), axis=1)
        clutter = rs.uniform((1.0, 1.0, 0.3), (3.0, 2.5, 1.5), (1500, 3))
        perm = rs.permutation(7500)
        xyz = np.ascontiguousarray(np.concatenate([floor, wall_x, wall_y, clutter])[perm], dtype=F32)
        xyz.setflags(write=False)
        _cases["room"] = (xyz, np.repeat(np.arange(4), [3000, 1500, 1500, 1500])[perm])
    return _cases["room"]


def room_twin():
    if "room" not in _twins:
        from randlanet.utils.planes import segment_planes_host
        _twins["room"] = _frozen(segment_planes_host(room()[0], **ROOM))
    return _twins["room"]


# -------------------------------------------------------------------------------------------------------- yardstick
def _hypothesis(pts, triple):
    """One hypothesis by np.float32 scalars, the contract of utils/planes.py written out once more: (4,) float32, NaN when
    invalid (without the axis rule)."""
    p0, p1, p2 = (pts[int(i)] for i in triple)
    with np.errstate(all="ignore"):
        e1 = [F32(p1[a] - p0[a]) for a in range(3)]
        e2 = [F32(p2[a] - p0[a]) for a in range(3)]
        c = [F32(F32(e1[1] * e2[2]) - F32(e1[2] * e2[1])), F32(F32(e1[2] * e2[0]) - F32(e1[0] * e2[2])),
             F32(F32(e1[0] * e2[1]) - F32(e1[1] * e2[0]))]
        l2 = F32(F32(F32(c[0] * c[0]) + F32(c[1] * c[1])) + F32(c[2] * c[2]))
        if not (l2 > 0 and np.isfinite(l2)):
            return np.full(4, np.nan, F32)
        r = F32(np.sqrt(l2))
        n = [F32(c[a] / r) for a in range(3)]
        d = F32(-F32(F32(F32(n[0] * p0[0]) + F32(n[1] * p0[1])) + F32(n[2] * p0[2])))
    return np.array(n + [d], F32)


def _inliers(pts, plane, thr, scalar):
    """(M,) bool by the score rule: point by point with np.float32 scalars, or - the larger cases - column by column."""
    if not scalar:
        x, y, z = (np.ascontiguousarray(pts[:, a]) for a in range(3))
        with np.errstate(all="ignore"):
            t = plane[0] * x
            t = t + plane[1] * y
            t = t + plane[2] * z
            t = t + plane[3]
        assert t.dtype == F32
        return ~(np.abs(t) > thr) & ~np.isnan(t)
    out = np.zeros(pts.shape[0], bool)
    with np.errstate(all="ignore"):
        for i, (x, y, z) in enumerate(pts):
            s = F32(F32(F32(F32(plane[0] * x) + F32(plane[1] * y)) + F32(plane[2] * z)) + plane[3])
            out[i] = abs(s) <= thr
    return out


def yardstick(name):
    """dict(hypotheses, counts, best, first_inlier - the mask of the best hypothesis -, mean, cov - the float64 moments of
    those inliers by boxes.fixed_sums -, normal - the eigenvector of the smallest eigenvalue by numpy's eigh, an independent
    solver that is close to, not bit-equal with, the contract's Jacobi sweeps), computed once."""
    if name not in _yards:
        from randlanet.utils.boxes import fixed_sums
        pts, kw = case(name)
        scalar = name in SCALAR
        thr = F32(kw["threshold"])
        M = pts.shape[0]
        tri = kw["triples"] if "triples" in kw else np.random.default_rng(kw["seed"]).integers(0, M, size=(kw["iterations"], 3),
                                                                                                dtype=np.int64)
        hyp = np.stack([_hypothesis(pts, t) for t in tri])
        if "axis" in kw:
            ax = np.asarray(kw["axis"], np.float64)
            ax = (ax / np.sqrt(ax @ ax)).astype(F32)
            cos_min = F32(np.cos(np.radians(np.float64(kw["max_angle"]))))
            for h in hyp:
                dot = F32(F32(F32(h[0] * ax[0]) + F32(h[1] * ax[1])) + F32(h[2] * ax[2]))
                if not abs(dot) >= cos_min:
                    h[:] = np.nan
        counts = np.array([int(_inliers(pts, h, thr, scalar).sum()) for h in hyp], np.int32)
        best = -1
        for t in range(counts.shape[0]):
            if counts[t] > (counts[best] if best >= 0 else 0):
                best = t
        out = dict(hypotheses=hyp, counts=counts, best=best)
        if best >= 0:
            inl = _inliers(pts, hyp[best], thr, scalar)
            n = np.array([int(inl.sum())])
            P = pts[inl].astype(np.float64)
            mean = fixed_sums(P, n)[0] / np.float64(n[0])
            d = P - mean
            prod = np.stack([d[:, a] * d[:, b] for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], axis=1)
            cov = fixed_sums(prod, n)[0] / np.float64(n[0])
            full = np.array([[cov[0], cov[1], cov[2]], [cov[1], cov[3], cov[4]], [cov[2], cov[4], cov[5]]])
            out.update(first_inlier=inl, mean=mean, cov=cov, normal=np.linalg.eigh(full)[1][:, 0])
        _yards[name] = out
    return _yards[name]


def fused_counts(name):
    """counts of the case's hypotheses with the score contracted into a chain of fused multiply-adds - s = fma(nz, z, fma(ny,
    y, nx * x)) + d, emulated in float64 (the product of two float32 values is exact there) -: what a kernel built without
    -ffp-contract=off, or on the MFMA units, would count."""
    pts, kw = case(name)
    hyp, thr = twin(name).hypotheses.astype(np.float64), F32(kw["threshold"])
    x, y, z = (pts[:, a].astype(np.float64) for a in range(3))
    out = np.zeros(hyp.shape[0], np.int32)
    with np.errstate(all="ignore"):
        for t, h in enumerate(hyp):
            s = (h[0] * x).astype(F32)
            s = (h[1] * y + s.astype(np.float64)).astype(F32)
            s = (h[2] * z + s.astype(np.float64)).astype(F32)
            s = s + F32(h[3])
            out[t] = int((np.abs(s) <= thr).sum())
    return out


# ------------------------------------------------------------------------------------------------------- comparisons
def bits(x):
    x = np.ascontiguousarray(x)
    return x.reshape(-1).view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def same_floats(g, w, dtype):
    """Bit for bit, but any NaN equals any NaN (numpy and the device write different payloads for `invalid`)."""
    g, w = np.asarray(g), np.asarray(w)
    return g.dtype == dtype and g.shape == w.shape and bool(((bits(g) == bits(w)) | (np.isnan(g) & np.isnan(w)).reshape(-1)).all())


def assert_same(got, want, what=""):
    """Every field of two PlaneFit: the float fields as bits, the integer fields exactly, types and shapes included."""
    assert same_floats(got.plane, want.plane, F32), (what, "plane", got.plane, want.plane)
    assert same_floats(got.hypotheses, want.hypotheses, F32), (what, "hypotheses")
    assert same_floats(got.centroid, want.centroid, np.float64), (what, "centroid", got.centroid, want.centroid)
    assert int(got.count) == int(want.count) and int(got.best) == int(want.best), (what, got.count, want.count, got.best, want.best)
    for f, dt in (("inlier", np.bool_), ("kept", np.int64), ("slot", np.int32), ("counts", np.int32)):
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == dt and g.shape == w.shape and np.array_equal(g, w), (what, f, g.dtype, g.shape, w.shape)


def assert_same_segmentation(got, want, what=""):
    assert same_floats(got.planes, want.planes, F32), (what, "planes", got.planes, want.planes)
    for f, dt in (("counts", np.int64), ("plane_id", np.int32), ("kept", np.int64), ("slot", np.int32)):
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == dt and g.shape == w.shape and np.array_equal(g, w), (what, f, g.dtype, g.shape, w.shape)
