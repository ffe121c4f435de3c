"""Shared inputs of the registration tests (test_registration_*): the seeded synthetic cases and the twin's result per case
(computed once, never modified).  A case is (source (Ms, 3) float32, target (Mt, 3) float32, keywords of icp_host)."""
import numpy as np

F32 = np.float32
AXIS = np.array([1.0, 2.0, 2.0]) / 3.0
ANGLE = 5.0                                         # degrees
SHIFT = np.array([0.03, -0.02, 0.01])
METRICS = ("point_to_plane", "point_to_point")
SIZES_S = (1, 63, 64, 65, 1023, 1024, 1025, 66561)  # 66561 = 65 chunks + 1: the second-level lanes 0 and 1 take two chunk sums
SIZES_T = (300, 3000)                               # the brute-force K-NN and the grid
_cases, _twins = {}, {}

GRID = tuple(f"{m}-{ms}-{mt}" for m in METRICS for ms in SIZES_S for mt in SIZES_T)
SPECIAL = ("duplicates", "zero_normals", "gated_out", "one_pair", "planted-point_to_plane-0.1", "planted-point_to_plane-0.05",
           "planted-point_to_point-0.1", "planted-point_to_point-0.05")
CASES = GRID + SPECIAL


def rotation(axis, degrees):
    a, t = np.asarray(axis, np.float64), np.radians(degrees)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def motion(degrees=ANGLE, shift=SHIFT, axis=AXIS):
    """The (4, 4) float64 transform that registers a moved source onto the target."""
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rotation(axis, degrees), shift
    return T


def moved_back(xyz, T):
    """xyz (float64) moved by the inverse of T: what icp has to undo."""
    return (xyz - T[:3, 3]) @ T[:3, :3]             # R^T (x - t), row by row


def corner(n=3000, seed=0):
    """A room corner inside the unit cube: a bumpy floor (n / 3 points), the walls x = 0 and y = 0 (n / 4 each) and a
    hemisphere of radius 0.2 on the floor (the rest); float64, permuted."""
    rs = np.random.RandomState(seed)
    nf, nw = n // 3, n // 4
    nh = n - nf - 2 * nw
    u = rs.uniform(0, 1, (nf, 2))
    floor = np.concatenate([u, (0.02 * np.sin(6 * u[:, 0]) * np.cos(5 * u[:, 1]))[:, None]], axis=1)
    v = rs.uniform(0, 1, (nw, 2))
    wall_x = np.stack((np.zeros(nw), v[:, 0], v[:, 1]), axis=1)
    v = rs.uniform(0, 1, (nw, 2))
    wall_y = np.stack((v[:, 0], np.zeros(nw), v[:, 1]), axis=1)
    d = rs.normal(size=(nh, 3))
    d[:, 2] = np.abs(d[:, 2])
    dome = np.array([0.55, 0.5, 0.0]) + 0.2 * d / np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([floor, wall_x, wall_y, dome])[rs.permutation(n)]


def _f32(x):
    x = np.ascontiguousarray(x, dtype=F32)
    x.setflags(write=False)
    return x


def case(name):
    if name not in _cases:
        kw = dict(max_distance=0.1, iterations=30)
        if name.startswith("planted-"):
            _, metric, md = name.split("-")
            tgt = corner(3000, 0)
            src = moved_back(tgt[np.random.RandomState(1).permutation(3000)[:1500]], motion())
            kw = dict(max_distance=float(md), metric=metric, iterations=30)
        elif name in GRID:
            metric, ms, mt = name.split("-")
            ms, mt = int(ms), int(mt)
            rs = np.random.RandomState(ms * 7 + mt)
            tgt = corner(mt, mt)
            src = moved_back(tgt[rs.randint(0, mt, ms)] + rs.normal(0, 0.002, (ms, 3)), motion(2.0, 0.4 * SHIFT))
            kw = dict(max_distance=0.08, metric=metric, iterations=3 if ms > 2000 else 6)
        elif name == "duplicates":      # every target point three times, 1000 apart: the lowest index wins every tie
            base = corner(1000, 5)
            tgt = np.concatenate([base, base, base])
            src = moved_back(base[::2], motion(1.0, 0.2 * SHIFT))
            kw = dict(max_distance=0.1, metric="point_to_point", iterations=4)
        elif name == "zero_normals":    # every third target normal is zero: zeros in the sums, still a pair
            tgt = corner(2000, 6)
            src = moved_back(tgt[::2], motion(1.0, 0.2 * SHIFT))
            from randlanet.utils.normals import estimate_normals_host
            nrm = estimate_normals_host(tgt.astype(F32), 12).normals.copy()
            nrm[::3] = 0.0
            kw = dict(max_distance=0.1, target_normals=_f32(nrm), iterations=4)
        elif name == "gated_out":       # the source lies 10 away: no pair, degenerate at once
            tgt = corner(1500, 7)
            src = tgt[:700] + np.array([10.0, 0.0, 0.0])
            kw = dict(max_distance=0.1, iterations=5)
        elif name == "one_pair":        # exactly one source point inside the gate
            tgt = corner(1500, 8)
            src = tgt[:1100] + np.array([0.0, 0.0, 7.0])
            src[1030] = tgt[17] + np.array([0.001, 0.0, 0.002])
            kw = dict(max_distance=0.05, iterations=5, min_pairs=1)
        else:
            raise KeyError(name)
        _cases[name] = (_f32(src), _f32(tgt), kw)
    return _cases[name]


def _frozen(res):
    for a in res:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


def twin(name):
    """RegistrationResult of the numpy twin for the case (computed once)."""
    if name not in _twins:
        from randlanet.utils.registration import icp_host
        src, tgt, kw = case(name)
        _twins[name] = _frozen(icp_host(src, tgt, **kw))
    return _twins[name]


# ------------------------------------------------------------------------------------------------------- Model.predict_views
KW = dict(votes=1, batch_size=4, seed=2)            # the predict_scene keywords of the Model tests


def views3():
    """Three overlapping views of one corner (700, 600 and 500 of its 1200 points), the second and third in frames of
    their own: 2 degrees and 0.3 * SHIFT, 3 degrees and 0.5 * SHIFT away."""
    tgt = corner(1200, 11)
    rs = np.random.RandomState(2)
    a = tgt[rs.permutation(1200)[:700]]
    b = moved_back(tgt[rs.permutation(1200)[:600]], motion(2.0, 0.3 * SHIFT))
    c = moved_back(tgt[rs.permutation(1200)[:500]], motion(3.0, 0.5 * SHIFT))
    return [a.astype(F32), b.astype(F32), c.astype(F32)]


def by_hand(model, views, settings, to, device):
    """predict_views restated with the public icp and predict_scene (np.random seeded with 5 before the votes):
    (confidences (C, sum of M_v), transformations (V, 4, 4), merged xyz)."""
    from dataclasses import asdict
    from randlanet.utils import registration as R
    moved, T = [views[0]], [np.eye(4)]
    for v in range(1, len(views)):
        target = moved[0] if to == "first" else moved[v - 1]
        res = R.icp(views[v], target, init=T[v - 1] if to == "previous" else None, device=device, **asdict(settings))
        moved.append(res.transformed)
        T.append(res.transformation)
    np.random.seed(5)
    out = model.predict_scene(np.concatenate(moved), **KW)
    return out, np.array(T), np.concatenate(moved)


def pose_error(T, want):
    """(rotation error in degrees, translation error) of T against `want`, both (4, 4)."""
    dR = T[:3, :3] @ want[:3, :3].T
    s = 0.5 * np.linalg.norm([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])      # sin: exact near 0
    angle = np.degrees(np.arctan2(s, (np.trace(dR) - 1.0) / 2.0))
    return float(angle), float(np.linalg.norm(T[:3, 3] - want[:3, 3]))


def bits(x):
    x = np.ascontiguousarray(x)
    return x.reshape(-1).view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def assert_same(got, want, what=""):
    """Every field of two RegistrationResult: the float fields as bits, the others exactly, types and shapes included."""
    for f, dt in (("transformation", np.float64), ("history", np.float64), ("transformed", F32)):
        g, w = getattr(got, f), getattr(want, f)
        assert isinstance(g, np.ndarray) and g.dtype == dt and g.shape == w.shape, (what, f, g.dtype, g.shape, w.shape)
        assert np.array_equal(bits(g), bits(w)), (what, f, np.flatnonzero(bits(g) != bits(w))[:8])
    for f in ("fitness", "inlier_rmse"):
        assert np.float64(getattr(got, f)).tobytes() == np.float64(getattr(want, f)).tobytes(), (what, f, getattr(got, f), getattr(want, f))
    assert (got.count, got.updates, got.status) == (want.count, want.updates, want.status), (what, got[3:6], want[3:6])
    g, w = got.correspondence, want.correspondence
    assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w), (what, "correspondence")
