"""Normals and curvature on the host: the numpy twin (utils/normals.py) against numpy.linalg.eigh on the cases of
tests/normals_inputs.py, every orientation rule, every refusal, the layout of normal_features and the host loader's
rotation of a feature triple.

The eigenvector bound: the twin's Jacobi leaves a backward error of a few units in the last place of C, and the first-order
perturbation of an eigenvector by an error E is |E| / gap, so with g = (w_1 - w_0) / w_2 the relative gap of the smallest
eigenvalue the sine of the angle between the twin's normal and eigh's is bounded by 64 * 2^-52 / g (64 units in the last
place; a prototype measured sin * g <= 6e-16 = 2.7 units, the run of this file prints what it sees), and the curvature - an
eigenvalue over the trace - is within 64 * 2^-52 of eigh's w_0 / sum(w).  Both are compared in float64, before the one
rounding to float32.  Points with g < 1e-4 may be left out, at most 1 % of a case, and none on the three random cases."""
import numpy as np
import pytest

import normals_inputs as ni

F32 = np.float32
EPS = 2.0 ** -52
BOUND = 64 * EPS
MIN_GAP = 1e-4


def _pre_rounding(cname):
    """(n (M, 3), curvature (M,)) float64 of the twin before orientation and rounding, and the covariances they come from."""
    from randlanet.utils import normals as N
    C = ni.covariances(cname)
    n, curv = N.smallest(*N.jacobi(C))
    assert n.dtype == curv.dtype == np.float64
    return n, curv, C


# ------------------------------------------------------------------------------------------------ (a) against eigh
@pytest.mark.parametrize("cname", list(ni.CLOUDS))
def test_covariances_follow_an_independent_knn(cname):
    """The twin's covariances against the same definition over an all-pairs numpy K-NN, summed in extended precision.
    Bound per entry (u = 2^-53, P = the largest |coordinate|, k terms added one by one): the centroid is off by at most
    k u P, a difference by that plus u |d|, so C_ab by u (k P (sqrt(C_aa) + sqrt(C_bb)) + (k + 3) sqrt(C_aa C_bb)); twice
    that is asserted."""
    xyz, k = ni.cloud(cname), ni.CLOUDS[cname]
    C = ni.covariances(cname)
    assert C.shape == (xyz.shape[0], 6) and C.dtype == np.float64
    P = xyz[ni.brute_knn(xyz, k)].astype(np.longdouble)
    d = P - P.mean(axis=1, keepdims=True)
    u, big = 2.0 ** -53, float(np.abs(xyz).max())
    diag = {0: C[:, 0], 1: C[:, 3], 2: C[:, 5]}
    e = 0
    for a in range(3):
        for b in range(a, 3):
            want = (d[:, :, a] * d[:, :, b]).mean(axis=1)
            sa, sb = np.sqrt(diag[a]), np.sqrt(diag[b])
            tol = 2 * u * (k * big * (sa + sb) + (k + 3) * sa * sb)
            err = np.abs(C[:, e] - want).astype(np.float64)
            assert (err <= tol).all(), (cname, a, b, float(err.max()), float(tol[err > tol][0]))
            e += 1


@pytest.mark.parametrize("cname", [c for c in ni.CLOUDS if c != "line"])
def test_twin_against_eigh(cname):
    from randlanet.utils import normals as N
    n, curv, C = _pre_rounding(cname)
    M = C.shape[0]
    w, E = np.linalg.eigh(ni.full_matrix(C))
    flat = w[:, 2] <= 0.0                                   # coincident neighbourhoods: checked for their defined output
    if cname == "coincident":
        assert int(flat.sum()) == 40
        assert not n[flat].any() and not curv[flat].any()
    else:
        assert not flat.any()
    with np.errstate(all="ignore"):
        g = (w[:, 1] - w[:, 0]) / w[:, 2]
    use = ~flat & (g >= MIN_GAP)
    left_out = int((~flat & ~use).sum())
    assert left_out <= 0.01 * M and (cname not in ni.RANDOM or left_out == 0), (cname, left_out, float(g[~flat].min()))
    sin = np.linalg.norm(np.cross(n[use], E[use][:, :, 0]), axis=1)
    ref = w[use, 0] / w[use].sum(axis=1)
    cerr = np.abs(curv[use] - ref)
    print(f"{cname}: {int(use.sum())} of {M} points, smallest gap {float(g[use].min()):.3g}, max sin*g "
          f"{float((sin * g[use]).max()) / EPS:.2f} ulp, max curvature error {float(cerr.max()) / EPS:.2f} ulp")
    assert (sin <= BOUND / g[use]).all(), (cname, float((sin * g[use]).max()))
    assert (cerr <= BOUND).all(), (cname, float(cerr.max()))
    assert (np.abs(np.linalg.norm(n[use], axis=1) - 1.0) <= 16 * EPS).all()      # 18 rotations keep V orthonormal
    # the public twin is these values, oriented and rounded once
    for v in ("up", "origin"):
        res = ni.twin(f"{cname}-{v}")
        assert res.normals.dtype == res.curvature.dtype == F32 and res.normals.shape == (M, 3) and res.curvature.shape == (M,)
        assert np.array_equal(np.abs(res.normals), np.abs(n.astype(F32)))
        assert np.array_equal(res.curvature, curv.astype(F32))
        assert ((res.curvature >= 0) & (res.curvature <= F32(1 / 3) + F32(1e-7))).all()


def test_plane_is_exact():
    for v in ("up", "origin"):
        res = ni.twin(f"plane-{v}")
        sign = 1.0 if v == "up" else -1.0                   # the origin lies below the plane z = 1.75
        assert (res.normals == np.array([0.0, 0.0, sign], F32)).all() and not res.curvature.any()


def test_line_has_its_defined_output():
    """Every neighbourhood lies on one line: two eigenvalues vanish up to rounding, so any unit vector across the line
    serves as the normal; the curvature is zero up to rounding."""
    n, curv, C = _pre_rounding("line")
    direction = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    assert (np.abs(n @ direction) <= BOUND).all() and (np.abs(np.linalg.norm(n, axis=1) - 1.0) <= 16 * EPS).all()
    assert ((curv >= 0) & (curv <= BOUND)).all()


def test_three_points_share_one_neighbourhood():
    res = ni.twin("three_points-up")
    xyz = ni.cloud("three_points").astype(np.float64)
    want = np.cross(xyz[1] - xyz[0], xyz[2] - xyz[0])
    want /= np.linalg.norm(want)
    # the ranks differ per query, so the sums - and the last bits - may; the plane through three points does not
    assert np.allclose(np.abs(res.normals @ want), 1.0, atol=1e-6) and (res.curvature <= 1e-7).all()
    assert (res.normals[:, 2] > 0).all()


def test_query_blocks_do_not_show(monkeypatch):
    from randlanet.utils import normals as N
    xyz, k, vp = ni.case("surface_1000-origin")
    monkeypatch.setattr(N, "_QUERY_BLOCK", 333)
    ni.assert_same(N.estimate_normals_host(xyz, k, vp), ni.twin("surface_1000-origin"))
    assert np.array_equal(N.covariances_host(xyz, k), ni.covariances("surface_1000"))


# ------------------------------------------------------------------------------------------------ (b) orientation
def test_orientation_rules():
    from randlanet.utils.normals import orient
    n = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.6, 0.0, -0.8], [0.6, -0.8, 0.0], [-1.0, 0.0, 0.0], [1.0, 0.0, 0.0],
                  [0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0]])
    pts = np.zeros((9, 3), F32)
    pts[7:] = (3.0, 5.0, -2.0)
    # without a viewpoint: upward - the first non-zero of (n_z, n_y, n_x) decides
    up = orient(n, pts, None)
    want_up = np.array([[0, 0, 1], [0, 0, 1], [-0.6, 0, 0.8], [-0.6, 0.8, 0], [1, 0, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0],
                        [0, 1, 0]], np.float64)
    assert np.array_equal(up, want_up)
    assert not np.signbit(up[6]).any()                       # the zero normal is never negated
    # towards a viewpoint: s = n . (v - p) < 0 negates, s > 0 keeps, s == 0 falls back to upward
    v = np.array([0.0, 0.0, -4.0], F32)
    got = orient(n, pts, v)
    want = np.array([[0, 0, -1],          # s = -4
                     [0, 0, -1],
                     [0.6, 0, -0.8],      # s = 3.2
                     [-0.6, 0.8, 0],      # s = 0: upward
                     [1, 0, 0],           # s = 0: upward
                     [1, 0, 0],
                     [0, 0, 0],           # the zero normal: s = 0, nothing to negate
                     [0, -1, 0],          # w = (-3, -5, -2): s = -5
                     [0, -1, 0]], np.float64)         # s = 5
    assert np.array_equal(got, want) and not np.signbit(got[6]).any()


def test_orientation_through_the_public_function():
    from randlanet.utils.normals import estimate_normals_host
    xyz = ni.cloud("plane")
    for v, sign in (((0, 0, 5), 1.0), ((0, 0, -5), -1.0), ((9, 9, 1.75), 1.0)):       # the last one lies ON the plane: s == 0
        res = estimate_normals_host(xyz, 12, v)
        assert (res.normals == np.array([0, 0, sign], F32)).all(), v
    # a viewpoint flips exactly the normals that look away from it
    a, xyz = ni.twin("surface_1000-up"), ni.cloud("surface_1000")
    for v, some_stay in (((0.0, 0.0, 0.0), False), ((3.0, 0.0, 2.25), True)):             # below the surface; beside it
        b = ni.twin("surface_1000-origin") if not some_stay else estimate_normals_host(xyz, 16, v)
        s = (a.normals.astype(np.float64) * (np.array(v) - xyz.astype(np.float64))).sum(axis=1)
        flipped = (a.normals != b.normals).any(axis=1)
        assert np.array_equal(flipped, s < 0) and flipped.any() and flipped.all() != some_stay
        assert np.array_equal(np.where(flipped[:, None], -a.normals, a.normals), b.normals)
        assert np.array_equal(a.curvature, b.curvature)
    # the coincident neighbourhoods: zero normal, zero curvature, whatever the viewpoint
    for v in ("up", "origin"):
        res = ni.twin(f"coincident-{v}")
        same = (ni.cloud("coincident") == np.array([0.25, -1.5, 3.0], F32)).all(axis=1)
        assert int(same.sum()) == 40
        assert not res.normals[same].any() and not np.signbit(res.normals[same]).any() and not res.curvature[same].any()
        assert (np.abs(np.linalg.norm(res.normals[~same], axis=1) - 1) < 1e-6).all()


# ------------------------------------------------------------------------------------------------ (c) refusals
def test_refusals():
    from randlanet.utils.normals import covariances_host, estimate_normals, estimate_normals_host, normal_features
    xyz = ni.cloud("noise_300_k3")
    for fn in (estimate_normals_host, lambda *a: estimate_normals(*a, device="cpu"),
               lambda *a: normal_features(*a, device="cpu")):
        for bad in (xyz[:, :2], xyz[None], xyz.ravel(), np.zeros((0, 3), F32)):
            with pytest.raises(ValueError, match="estimate_normals: "):
                fn(bad, 3)
        for k in (2, 0, -1, 65, 2.5, True):
            with pytest.raises(ValueError, match="must be an integer in 3 .. 64"):
                fn(xyz, k)
        with pytest.raises(ValueError, match=r"M=15 points, outside k=16"):
            fn(xyz[:15], 16)
        for value in (np.nan, np.inf, -np.inf, 1e39):        # (1e39 is infinite in float32)
            broken = np.array(xyz, dtype=np.float64)
            broken[17, 1] = value
            with pytest.raises(ValueError, match="non-finite coordinates, first at point 17"):
                fn(broken, 3)
        for vp in ((0, 0), (0, 0, 0, 0), [[0, 0, 0]], (0, np.nan, 0), (np.inf, 0, 0), (1e39, 0, 0), "abc", 1.0):
            with pytest.raises(ValueError, match="viewpoint=.* must be three finite numbers"):
                fn(xyz, 3, vp)
    huge = np.lib.stride_tricks.as_strided(np.zeros(1, F32), shape=(2 ** 31 - 1, 3), strides=(0, 0))
    with pytest.raises(ValueError, match=r"M=2147483647 points, outside k=16 \.\. 2\^31 - 2"):
        estimate_normals_host(huge, 16)
    with pytest.raises(ValueError, match="must be an integer in 3 .. 64"):
        covariances_host(xyz, 65)
    # what is accepted: float64 and integer coordinates, a numpy integer k, a viewpoint as an array
    res = estimate_normals_host(xyz.astype(np.float64), np.int64(3), np.zeros(3))
    ni.assert_same(res, ni.twin("noise_300_k3-origin"))


# ------------------------------------------------------------------------------------------------ (d) layout
def test_normal_features_layout():
    from randlanet.utils.normals import normal_features
    xyz, k, vp = ni.case("duplicates-origin")
    f = normal_features(xyz, k, vp, device="cpu")
    want = ni.twin("duplicates-origin")
    assert f.shape == (xyz.shape[0], 4) and f.dtype == F32 and f.flags.c_contiguous
    assert np.array_equal(f[:, :3], want.normals) and np.array_equal(f[:, 3], want.curvature)
    # duplicated points have the same neighbours - ties go to the lower index for both - and so the same row
    _, first, inverse = np.unique(xyz, axis=0, return_index=True, return_inverse=True)
    assert np.array_equal(f, f[first[inverse.ravel()]])


# ------------------------------------------------------------------------------------------------ (e) host loaders
def test_host_loader_rotates_the_triple(monkeypatch):
    from randlanet.utils import augmentation as A
    from randlanet.utils.dataset import PointCloudPreprocessor, get_data_loader
    from randlanet.utils.normals import rotate_columns
    rs = np.random.RandomState(3)
    M, n, F, col = 500, 64, 5, 1
    xyz = rs.uniform(-1, 1, (M, 3))
    feat = rs.standard_normal((M, F)).astype(F32)
    lab = rs.randint(0, 4, M).astype(np.int64)
    drawn = []
    rotation = A._rotation
    monkeypatch.setattr(A, "_rotation", lambda *a: drawn.append(rotation(*a)) or drawn[-1])
    aug = A.AugmentationSettings(rotation_angle_variances=(0.5, 0.5, 0.5), rotation_angle_limits=(1.0, 1.0, 1.0))
    outs = []
    for c in (None, col):
        np.random.seed(9)
        outs.append(PointCloudPreprocessor([(xyz, feat, lab)], n, consistent_sampling=False, augmentation_settings=aug,
                                           normal_column=c).preprocess(xyz, feat, lab))
    (x0, f0, l0), (x1, f1, l1) = outs
    assert len(drawn) == 2 and np.array_equal(drawn[0], drawn[1])
    R = drawn[0]
    assert np.abs(R - np.eye(3)).max() > 0.05
    assert np.array_equal(x0, x1) and np.array_equal(l0, l1)                  # same draws, same coordinates
    other = [c for c in range(F) if not col <= c < col + 3]
    assert np.array_equal(f0[:, other], f1[:, other]) and f1.dtype == F32
    t = f0[:, col:col + 3].astype(np.float64)
    want = np.stack([(t[:, 0] * R[r, 0] + t[:, 1] * R[r, 1]) + t[:, 2] * R[r, 2] for r in range(3)], axis=1).astype(F32)
    assert np.array_equal(f1[:, col:col + 3], want)
    # the product the coordinates go through: (x - c) . R^T
    assert np.allclose(rotate_columns(t, 0, R), t @ R.T, rtol=0, atol=1e-15)
    # without augmentation nothing turns; a triple that does not fit is refused
    plain = [PointCloudPreprocessor([(xyz, feat, lab)], n, normal_column=c).preprocess(xyz, feat, lab) for c in (None, col)]
    assert np.array_equal(plain[0][1], plain[1][1]) and len(drawn) == 2
    np.random.seed(9)
    with pytest.raises(ValueError, match="normal_column=3"):
        PointCloudPreprocessor([(xyz, feat, lab)], n, augmentation_settings=aug, normal_column=3).preprocess(xyz, feat, lab)
    np.random.seed(9)
    inp, _, _ = next(iter(get_data_loader([(xyz, feat, lab)], n, 1, consistent_sampling=False, augmentation_settings=aug,
                                          normal_column=col)))
    assert np.array_equal(inp[0, :, 3:].numpy(), f1)


def test_loaders_check_normal_column():
    from randlanet.utils.device_dataset import check_normal_column
    assert check_normal_column(None, 0) == 0 and check_normal_column(0, 3) == 1 and check_normal_column(2, 5) == 3
    for c, F in ((0, 2), (3, 5), (-1, 5), (1.5, 6)):
        with pytest.raises(ValueError, match="normal_column="):
            check_normal_column(c, F)
