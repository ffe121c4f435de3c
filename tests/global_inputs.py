"""Seeded inputs of the global-registration tests (FPFH descriptors, matching, RANSAC over correspondences), with the numpy
twin's result cached per case: the CPU tests check the twin against independent restatements, the GPU tests check the device
against the twin bit for bit."""
import numpy as np

import registration_inputs as RI

F32 = np.float32
AXIS = RI.AXIS
SHIFT = np.array([0.4, -0.3, 0.2])
MAX_DISTANCE = 0.05
VIEWPOINT = np.array([1.2, 1.1, 1.5])               # the sensor, in the target's frame: in front of the corner, above it
ITERATIONS = 65536
_cache = {}

# name -> (degrees, noise sigma, target points, source points)
PLANTED = {"rot40": (40.0, 0.0, 3000, 1500), "rot120": (120.0, 0.0, 3000, 1500), "rot175": (175.0, 0.0, 3000, 1500),
           "rot120-noise": (120.0, 0.002, 3000, 1500), "rot40-small": (40.0, 0.0, 1200, 700)}

# The conditions of the issue on the twin's global estimate, every planted case: rotation within 10 degrees, translation
# within 0.1 (a tenth of the scene's size).
GLOBAL_ROTATION_CAP, GLOBAL_TRANSLATION_CAP = 10.0, 0.1
# After icp(init=global.transformation, max_distance=0.05) on the twin: the measured final errors (degrees, translation) per
# case, and the asserted bounds = twice the worst measured value.
MEASURED_FINAL = {"rot40": (1.0e-06, 1.2e-08), "rot120": (2.0e-06, 2.9e-08), "rot175": (2.1e-06, 3.8e-08),
                  "rot120-noise": (2.242e-02, 1.32e-04), "rot40-small": (6.5e-07, 1.9e-08)}
FINAL_ROTATION_BOUND, FINAL_TRANSLATION_BOUND = 2 * 2.242e-02, 2 * 1.32e-04        # the noisy case sets both
# (the twin's global estimates themselves were 0.98 to 2.04 degrees and 0.011 to 0.025 from the planted motions, and
# icp(init=identity) ended 14.1 to 158.8 degrees away)


def scene(n=3000, seed=0):
    """registration_inputs.corner (half of the points) plus what makes it less self-similar: a small dome on the wall x = 0,
    the top and one side of a box on the floor, and a tilted slab; inside the unit cube, float64, permuted."""
    rs = np.random.RandomState(seed + 1000)
    nc = n // 2
    nd, nb, ns = n // 10, n // 5, n - n // 2 - n // 10 - n // 5
    base = RI.corner(nc, seed)
    d = rs.normal(size=(nd, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:, 0] = np.abs(d[:, 0])
    dome = np.array([0.0, 0.7, 0.6]) + 0.12 * d
    u = rs.uniform(0, 1, (nb, 2))
    top = np.stack((0.1 + 0.25 * u[:, 0], 0.55 + 0.3 * u[:, 1], np.full(nb, 0.18)), axis=1)
    side = np.stack((0.1 + 0.25 * u[:, 0], np.full(nb, 0.55), 0.18 * u[:, 1]), axis=1)
    box = np.where((np.arange(nb) % 2 == 0)[:, None], top, side)
    u = rs.uniform(0, 1, (ns, 2))
    slab = np.stack((0.55 + 0.35 * u[:, 0], 0.5 + 0.4 * u[:, 1], 0.3 + 0.4 * u[:, 0] + 0.15 * u[:, 1]), axis=1)
    pts = np.concatenate((base, dome, box, slab))
    return pts[rs.permutation(n)]


def planted(name):
    """(source float32, target float32, the (4, 4) motion that registers the source onto the target).  The source is what a
    sensor at VIEWPOINT saw, in a frame of its own: planted_keywords gives that position in both frames."""
    key = ("planted", name)
    if key not in _cache:
        degrees, sigma, nt, ns = PLANTED[name]
        tgt = scene(nt, 0)
        T = RI.motion(degrees, SHIFT)
        rs = np.random.RandomState(7)
        src = RI.moved_back(tgt[rs.permutation(nt)[:ns]], T)
        if sigma:
            src = src + rs.normal(scale=sigma, size=src.shape)
        _cache[key] = (RI._f32(src), RI._f32(tgt), T)
    return _cache[key]


def planted_keywords(name):
    T = planted(name)[2]
    return dict(max_distance=MAX_DISTANCE, k=30, normals=16, iterations=ITERATIONS, seed=0, target_viewpoint=VIEWPOINT,
                source_viewpoint=RI.moved_back(VIEWPOINT[None], T)[0])


def planted_twin(name):
    """GlobalRegistrationResult of the numpy twin for the planted case (computed once)."""
    key = ("twin", name)
    if key not in _cache:
        from randlanet.utils.registration import global_registration_host
        src, tgt, _ = planted(name)
        _cache[key] = RI._frozen(global_registration_host(src, tgt, **planted_keywords(name)))
    return _cache[key]


# ---------------------------------------------------------------------------------------------------------- descriptors
DESCRIPTOR_SPECIALS = ("duplicates", "zero_normals", "collinear", "along_normal", "planar")


def descriptor_case(name):
    """(xyz float32, normals float32 or None, k) of a descriptor case: "M-k" of the grid, or a special."""
    key = ("descriptor", name)
    if key in _cache:
        return _cache[key]
    nrm = None
    if name in DESCRIPTOR_SPECIALS:
        rs = np.random.RandomState(len(name))
        k = 16
        pts = scene(400, 3)
        if name == "duplicates":                        # d2 = 0 among the ranks 1 .. k: 40 points appear three times
            pts = np.concatenate((pts, pts[:40], pts[:40]))
        elif name == "zero_normals":
            nrm = rs.normal(size=pts.shape)
            nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
            nrm[::7] = 0.0
        elif name == "collinear":                       # every d is parallel to the line and so is the normal: lv2 = 0
            pts = np.outer(np.arange(200) * 0.25, [1.0, 0.0, 0.0])
            nrm = np.tile([1.0, 0.0, 0.0], (200, 1))
        elif name == "along_normal":                    # pairs of points one exactly above the other, normals (0, 0, 1)
            g = np.stack(np.meshgrid(np.arange(10) * 0.5, np.arange(10) * 0.5), axis=-1).reshape(-1, 2)
            pts = np.concatenate((np.c_[g, np.zeros(100)], np.c_[g, np.full(100, 0.125)]))
            nrm = np.tile([0.0, 0.0, 1.0], (200, 1))
        elif name == "planar":                          # an exactly planar cloud with estimated normals
            pts = np.c_[rs.randint(0, 1024, (300, 2)) / 1024.0, np.zeros(300)]
    else:
        M, k = (int(v) for v in name.split("-"))
        pts = scene(max(M, 40), M + k)[:M] if M >= 40 else np.random.RandomState(M + k).uniform(0, 1, (M, 3))
    _cache[key] = (RI._f32(pts), None if nrm is None else RI._f32(nrm), k)
    return _cache[key]


def descriptor_twin(name):
    key = ("descriptor_twin", name)
    if key not in _cache:
        from randlanet.utils.features import fpfh_host
        pts, nrm, k = descriptor_case(name)
        _cache[key] = RI._frozen(fpfh_host(pts, k=k, normals=nrm, normal_k=min(16, pts.shape[0])))
    return _cache[key]


# ------------------------------------------------------------------------------------------------------------- matching
def codes(Ms, Mt):
    """(code_source (Ms, 36), code_target (Mt, 36)) uint8: random rows of a small alphabet - so that equal distances are
    common -, all-0 against all-255 rows (the largest distance), duplicated target rows (ties) and source rows equal to a
    target row (distance 0)."""
    key = ("codes", Ms, Mt)
    if key not in _cache:
        rs = np.random.RandomState(Ms * 13 + Mt)
        cs = np.zeros((Ms, 36), np.uint8)
        ct = np.zeros((Mt, 36), np.uint8)
        cs[:, :33] = rs.randint(0, 4, (Ms, 33)) * 85
        ct[:, :33] = rs.randint(0, 4, (Mt, 33)) * 85
        if Mt >= 3:
            ct[Mt // 2] = ct[0]                         # a tie: the lower index has to win
            ct[Mt - 1, :33] = 255
        cs[0, :33] = 0                                  # against the all-255 row: 33 * 255^2 when Mt == 1 ... the maximum
        if Mt == 1:
            ct[0, :33] = 255
        if Ms >= 3:
            cs[Ms // 2] = ct[Mt // 2]                   # distance 0, and a tie with row 0 of the target when Mt >= 3
            cs[Ms - 1] = ct[Mt - 1]
        cs.setflags(write=False)
        ct.setflags(write=False)
        _cache[key] = (cs, ct)
    return _cache[key]


# --------------------------------------------------------------------------------------------------------------- RANSAC
def ransac_case(T, C, special=None):
    """(source (C, 3), target (Mt, 3), corr (C,), triples (T, 3), edge_similarity, max_distance): a moved copy of a scene
    with a third of the correspondences wrong."""
    key = ("ransac", T, C, special)
    if key not in _cache:
        rs = np.random.RandomState(T * 31 + C)
        Mt = C + 5
        tgt = scene(max(Mt, 40), C)[:Mt]
        M = RI.motion(75.0, SHIFT)
        true = rs.permutation(Mt)[:C]
        src = RI.moved_back(tgt[true], M)
        wrong = rs.uniform(size=C) < 1.0 / 3.0
        corr = np.where(wrong, rs.randint(0, Mt, C), true).astype(np.int64)
        tri = rs.randint(0, C, (T, 3)).astype(np.int64)
        es = 0.9
        if special == "repeated":
            tri[::2, 1] = tri[::2, 0]
            tri[1::4, 2] = tri[1::4, 1]
        elif special == "collinear":                    # the source on a line: every cross product is zero
            src = np.outer(np.arange(C) * 0.01, [1.0, 2.0, 2.0])
            es = 0.0
        elif special == "rejected":                     # the source shrunk to half, every correspondence right: no edge is similar
            src, corr = 0.5 * src, true.astype(np.int64)
        _cache[key] = (RI._f32(src), RI._f32(tgt), corr, tri, es, 0.02)
    return _cache[key]


def ransac_twin(T, C, special=None):
    key = ("ransac_twin", T, C, special)
    if key not in _cache:
        from randlanet.utils import registration as R
        src, tgt, corr, tri, es, md = ransac_case(T, C, special)
        chk = R.check_global_parameters(md, iterations=T, edge_similarity=es)
        _cache[key] = RI._frozen(R._global_checked_host(src, tgt, corr, tri, chk))
    return _cache[key]


def assert_same_global(got, want, what=""):
    """Every field of two GlobalRegistrationResult: the float fields as bits (NaN positions included), the others exactly."""
    for f, dt in (("transformation", np.float64), ("hypotheses", F32), ("sums", np.float64)):
        g, w = getattr(got, f), getattr(want, f)
        assert isinstance(g, np.ndarray) and g.dtype == dt and g.shape == w.shape, (what, f, g.dtype, g.shape, w.shape)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, f, "NaN positions")
        assert np.array_equal(RI.bits(np.nan_to_num(g)), RI.bits(np.nan_to_num(w))), (what, f)
    for f, dt in (("inlier", np.bool_), ("correspondence", np.int64), ("counts", np.int32)):
        g, w = getattr(got, f), getattr(want, f)
        assert isinstance(g, np.ndarray) and g.dtype == dt and g.shape == w.shape and np.array_equal(g, w), (what, f)
    assert (got.count, got.best, got.status) == (want.count, want.best, want.status), (what, got.count, got.best, got.status)
    assert np.float64(got.fitness).tobytes() == np.float64(want.fitness).tobytes(), (what, "fitness")


# ------------------------------------------------------------------------------------------------------- Model.predict_views
def views():
    """Three views of one scene (800, 700 and 600 of its 1200 points), the second and third 120 and -60 degrees away, and
    the motions that bring them back."""
    tgt = scene(1200, 0)
    rs = np.random.RandomState(4)
    a = tgt[rs.permutation(1200)[:800]]
    b = RI.moved_back(tgt[rs.permutation(1200)[:700]], RI.motion(120.0, SHIFT))
    c = RI.moved_back(tgt[rs.permutation(1200)[:600]], RI.motion(-60.0, 0.5 * SHIFT))
    return [a.astype(F32), b.astype(F32), c.astype(F32)], [np.eye(4), RI.motion(120.0, SHIFT), RI.motion(-60.0, 0.5 * SHIFT)]


def views_by_hand(model, views, icp, settings, to, device, vps):
    """predict_views(global_init=...) restated with the public grid_subsample, global_registration, icp and predict_views."""
    from dataclasses import asdict
    from randlanet.utils import registration as R
    from randlanet.utils.grid import grid_subsample
    moved, T, poses = [views[0]], [np.eye(4)], [None]
    for v in range(1, len(views)):
        w = 0 if to == "first" else v - 1
        res = R.global_registration(grid_subsample(views[v], cell=settings.voxel, device=device).xyz,
                                    grid_subsample(moved[w], cell=settings.voxel, device=device).xyz,
                                    max_distance=1.5 * settings.voxel, k=settings.k, normals=settings.normals,
                                    iterations=settings.iterations, seed=settings.seed, edge_similarity=settings.edge_similarity,
                                    source_viewpoint=vps[v], target_viewpoint=T[w][:3, :3] @ vps[w] + T[w][:3, 3], device=device)
        assert res.status == "refined"
        poses.append(res.transformation)
        fine = R.icp(views[v], moved[w], init=res.transformation, device=device, **asdict(icp))
        moved.append(fine.transformed)
        T.append(fine.transformation)
    np.random.seed(5)
    return model.predict_views(views, icp=icp, to=to, poses=poses, **RI.KW), poses
