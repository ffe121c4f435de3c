"""The numpy twins of the global registration (utils/features.py, utils/registration.py) against independent restatements:
the descriptor against a float64 per-pair one with true angles, the matching against an int64 brute force, the hypotheses and
Kabsch against their geometry, every refusal, the planted cases, and Model.predict_views(global_init=...) on a CPU-placed model
against the same steps done by hand."""
import numpy as np
import pytest

import global_inputs as gi
import registration_inputs as ri

F32 = np.float32


# ------------------------------------------------------------------------------------------------------- (a) descriptor
def _pairs64(pts, nrm, idx):
    """The Darboux features of every (point, rank 1 .. k) pair in float64, with true angles: (f1, f2, theta)."""
    p, n = pts.astype(np.float64), nrm.astype(np.float64)
    i = np.broadcast_to(np.arange(p.shape[0])[:, None], idx[:, 1:].shape)
    j = idx[:, 1:]
    d = p[j] - p[i]
    dn = d / np.linalg.norm(d, axis=-1, keepdims=True)
    u = n[i]
    v = np.cross(dn, u)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    w = np.cross(u, v)
    f1 = (v * n[j]).sum(-1)
    f2 = (u * dn).sum(-1)
    return f1, f2, (u * n[j]).sum(-1), (w * n[j]).sum(-1)


@pytest.mark.parametrize("name", ("3000-16", "1025-63", "1023-2"))
def test_linear_bins_equal_a_float64_restatement(name):
    from randlanet.utils import features as F
    pts, _, k = gi.descriptor_case(name)
    twin = gi.descriptor_twin(name)
    idx, d2 = F._knn_rows(pts, k + 1)
    f1, f2, x, y = _pairs64(pts, twin.normals, idx)
    t1, t2 = (f1 + 1.0) * 5.5, (f2 + 1.0) * 5.5
    sure = (np.abs(t1 - np.round(t1)) > 1e-5 * 5.5) & (np.abs(t2 - np.round(t2)) > 1e-5 * 5.5)      # 1e-5 from a bin edge, in f
    assert (~sure).mean() < 0.01
    b1 = np.clip(np.floor(t1), 0, 10).astype(np.int64)
    b2 = np.clip(np.floor(t2), 0, 10).astype(np.int64)
    g1, g2, gx, gy, counted = F.pair_features_host(pts, twin.normals, np.broadcast_to(np.arange(pts.shape[0])[:, None], b1.shape),
                                                   idx[:, 1:], d2[:, 1:])
    assert counted.all()
    c1, c2, c3 = F.bins_host(g1, g2, gx, gy)
    assert np.array_equal(c1[sure], b1[sure]) and np.array_equal(c2[sure], b2[sure])
    # the pseudo-angle bin against its own definition in float64, where that is 1e-4 (in bins) away from an edge
    s = np.abs(x) + np.abs(y)
    r = y / s
    a = np.where(x > 0, 2.0 + r, np.where(y >= 0, 4.0 - r, -r))
    t3 = a * 2.75
    sure3 = np.abs(t3 - np.round(t3)) > 1e-4
    assert (~sure3).mean() < 0.01
    assert np.array_equal(c3[sure3], np.minimum(np.floor(t3), 10).astype(np.int64)[sure3])
    # and it is monotone in the true angle, from -pi to pi
    order = np.argsort(np.arctan2(y, x).ravel(), kind="stable")
    assert (np.diff(a.ravel()[order]) >= -1e-9).all()
    # the histograms count exactly these bins, and the descriptor sums to 100 per sub-histogram
    hist = np.zeros((pts.shape[0], 33), np.int64)
    rows = np.broadcast_to(np.arange(pts.shape[0])[:, None], c1.shape)
    for off, c in ((0, c1), (11, c2), (22, c3)):
        np.add.at(hist, (rows, off + c), 1)
    assert np.array_equal(hist, twin.spfh)
    sums = twin.descriptor.reshape(-1, 3, 11).sum(axis=2)
    assert np.abs(sums - 100.0).max() < 1e-3
    assert (twin.code[:, 33:] == 0).all() and np.array_equal(twin.code[:, :33], np.minimum(255, np.floor(twin.descriptor * F32(2.55) + F32(0.5))))


def test_descriptor_does_not_change_under_a_rigid_motion():
    """What the feature is for: the histograms of a moved copy differ in a few bins only (rounding at bin edges)."""
    from randlanet.utils.features import fpfh_host
    pts, _, _ = gi.descriptor_case("1025-16")
    twin = gi.descriptor_twin("1025-16")
    M = ri.motion(120.0, gi.SHIFT)
    moved = ri.moved_back(pts.astype(np.float64), M).astype(F32)
    nrm = (twin.normals.astype(np.float64) @ M[:3, :3]).astype(F32)
    other = fpfh_host(moved, k=16, normals=nrm)
    assert (other.spfh.astype(int) - twin.spfh).__abs__().sum() < 0.01 * twin.spfh.sum()


def test_descriptor_specials_are_what_they_claim():
    t = gi.descriptor_twin
    assert (t("collinear").spfh == 0).all() and (t("collinear").code == 0).all() and (t("collinear").descriptor == 0).all()
    assert (t("zero_normals").spfh[::7] == 0).all() and t("zero_normals").spfh[1].sum() > 0
    assert t("along_normal").spfh[:, :11].sum(axis=1).max() == 15
    assert t("duplicates").spfh[:40, :11].sum(axis=1).max() == 14
    for name in gi.DESCRIPTOR_SPECIALS:
        assert np.isfinite(t(name).descriptor).all()


# --------------------------------------------------------------------------------------------------------- (b) matching
@pytest.mark.parametrize("Ms,Mt", [(1, 1), (65, 63), (257, 1000), (1025, 4097)])
def test_matching_equals_an_int64_brute_force(Ms, Mt):
    from randlanet.utils.features import match_features_host
    cs, ct = gi.codes(Ms, Mt)
    idx, dist = match_features_host(cs, ct)
    d = ((cs.astype(np.int64)[:, None, :] - ct.astype(np.int64)[None, :, :]) ** 2).sum(axis=2)
    assert idx.dtype == np.int64 and dist.dtype == np.int32
    assert np.array_equal(idx, d.argmin(axis=1)) and np.array_equal(dist, d.min(axis=1))
    if Mt == 1:
        assert dist[0] == 33 * 255 * 255


# ----------------------------------------------------------------------------------------------------------- (c) RANSAC
def test_hypotheses_are_rotations_that_map_the_triangle_onto_its_image():
    from randlanet.utils import registration as R
    src, tgt, corr, tri, es, md = gi.ransac_case(1025, 1025)
    hyp = gi.ransac_twin(1025, 1025).hypotheses
    ok = ~np.isnan(hyp[:, 0])
    assert 100 < ok.sum() < 1025 and (np.isnan(hyp).all(axis=1) == ~ok).all()
    Rm = hyp[ok, :9].reshape(-1, 3, 3).astype(np.float64)
    t = hyp[ok, 9:].astype(np.float64)
    # nine float32 entries, each the sum of three products of unit-vector components that carry a few ulps each: 64 eps
    eps = float(np.finfo(F32).eps)
    assert np.abs(Rm @ Rm.transpose(0, 2, 1) - np.eye(3)).max() < 64 * eps
    assert np.abs(np.linalg.det(Rm) - 1.0).max() < 64 * eps
    a = [src[tri[ok, m]].astype(np.float64) for m in range(3)]
    b = [tgt[corr[tri[ok, m]]].astype(np.float64) for m in range(3)]
    q0 = np.einsum("tij,tj->ti", Rm, a[0]) + t
    assert np.abs(q0 - b[0]).max() < 64 * eps                                   # the first corner onto its image
    q1 = np.einsum("tij,tj->ti", Rm, a[1]) + t
    along = b[1] - b[0]
    along /= np.linalg.norm(along, axis=1, keepdims=True)
    off = (q1 - b[0]) - ((q1 - b[0]) * along).sum(1, keepdims=True) * along      # the second onto the ray through its image
    assert np.abs(off).max() < 256 * eps
    q2 = np.einsum("tij,tj->ti", Rm, a[2]) + t
    nb = np.cross(b[1] - b[0], b[2] - b[0])
    nb /= np.linalg.norm(nb, axis=1, keepdims=True)
    assert np.abs(((q2 - b[0]) * nb).sum(1)).max() < 256 * eps                   # the third into the image's plane
    # the edge test: a hypothesis is valid only when every pair of edges is within the similarity
    la = [np.linalg.norm(a[i] - a[j], axis=1) for i, j in ((1, 0), (2, 0), (2, 1))]
    lb = [np.linalg.norm(b[i] - b[j], axis=1) for i, j in ((1, 0), (2, 0), (2, 1))]
    for x, y in zip(la, lb):
        assert (np.minimum(x, y) / np.maximum(x, y) >= es - 1e-6).all()


def test_kabsch_recovers_a_planted_motion_from_exact_correspondences():
    from randlanet.utils import registration as R
    rs = np.random.RandomState(3)
    M = ri.motion(137.0, gi.SHIFT)
    b = rs.uniform(0, 1, (500, 3)).astype(F32)
    a = ri.moved_back(b.astype(np.float64), M)
    cols = np.concatenate((np.ones((500, 1)), a, b.astype(np.float64), (a[:, :, None] * b[:, None, :].astype(np.float64)).reshape(-1, 9)), axis=1)
    T = R.kabsch(cols.sum(axis=0))
    rot, tr = ri.pose_error(T, M)
    assert rot < 1e-5 and tr < 1e-7                                              # float32 targets: 6e-8 per coordinate
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-12
    mirror = cols.copy()                                                         # a reflected set still gives a rotation
    mirror[:, 4] = -mirror[:, 4]
    mirror[:, 7:16] = (a[:, :, None] * (b.astype(np.float64) * [-1, 1, 1])[:, None, :]).reshape(-1, 9)
    assert abs(np.linalg.det(R.kabsch(mirror.sum(axis=0))[:3, :3]) - 1.0) < 1e-12
    assert R.kabsch(np.full(16, np.nan)) is None


def test_ransac_specials():
    want = gi.ransac_twin(129, 1025, "repeated")
    assert np.isnan(want.hypotheses[::2]).all() and want.status == "refined"
    for sp, T, C in (("collinear", 65, 65), ("rejected", 1025, 1025)):
        want = gi.ransac_twin(T, C, sp)
        assert np.isnan(want.hypotheses).all() and want.status == "not_found" and want.best == -1 and not want.inlier.any()
        assert np.array_equal(want.transformation, np.eye(4)) and (want.sums == 0).all() and want.count == 0
    src, tgt, corr, tri, es, md = gi.ransac_case(65, 1024)
    want = gi.ransac_twin(65, 1024)
    M = ri.motion(75.0, gi.SHIFT)
    assert ri.pose_error(want.transformation, M)[0] < 1e-3 and want.count > 512
    assert want.sums[0] == want.counts[want.best] and np.array_equal(want.correspondence, corr)


# ---------------------------------------------------------------------------------------------------------- (d) refusals
def test_every_refusal_is_a_value_error_that_names_the_argument():
    from randlanet.utils import features as F
    from randlanet.utils import registration as R
    pts, _, _ = gi.descriptor_case("65-16")
    bad_cloud = pts.copy()
    bad_cloud[3, 1] = np.nan
    for kw, word in ((dict(k=1), "k"), (dict(k=64), "k"), (dict(k=2.5), "k"), (dict(k=True), "k"), (dict(normal_k=2), "normal_k"),
                     (dict(normal_k=65), "normal_k"), (dict(viewpoint=(0, 0)), "viewpoint"), (dict(viewpoint=(0, np.inf, 0)), "viewpoint"),
                     (dict(normals=np.zeros((64, 3))), "normals"), (dict(normals=np.full((65, 3), np.nan)), "normals")):
        with pytest.raises(ValueError, match=word):
            F.fpfh_host(pts, **kw)
    for cloud, word in ((pts[:16], "M=16"), (pts[:, :2], "shape"), (bad_cloud, "non-finite"), (pts[:10], "M=10")):
        with pytest.raises(ValueError, match=word):
            F.fpfh_host(cloud, k=16 if cloud.shape[0] != 10 else 2)
    code = np.zeros((4, 36), np.uint8)
    for cs, ct, word in ((code[:, :33], code, "code_source"), (code, code.astype(np.int32), "code_target"), (code[:0], code, "code_source")):
        with pytest.raises(ValueError, match=word):
            F.match_features_host(cs, ct)
    src, tgt, _ = gi.planted("rot40-small")
    good = dict(max_distance=0.05, iterations=8)
    for kw, word in ((dict(max_distance=0.0), "max_distance"), (dict(max_distance=np.nan), "max_distance"), (dict(k=1), "k"),
                     (dict(normals=2), "normals"), (dict(iterations=0), "iterations"), (dict(iterations=2 ** 20 + 1), "iterations"),
                     (dict(seed=-1), "seed"), (dict(seed="x"), "seed"), (dict(edge_similarity=1.5), "edge_similarity"),
                     (dict(edge_similarity=-0.1), "edge_similarity"), (dict(edge_similarity=None), "edge_similarity"),
                     (dict(source_viewpoint=(1, 2)), "viewpoint"), (dict(target_normals=np.zeros((3, 3))), "normals of target"),
                     (dict(source_normals=np.zeros((3, 3))), "normals of source"),
                     (dict(triples=np.zeros((4, 2), np.int64)), "triples"), (dict(triples=np.full((4, 3), 700)), "triples"),
                     (dict(triples=np.zeros((4, 3))), "triples")):
        with pytest.raises(ValueError, match=word):
            R.global_registration_host(src, tgt, **{**good, **kw})
    with pytest.raises(ValueError, match="source"):
        R.global_registration_host(src[:20], tgt, **good)
    with pytest.raises(ValueError, match="target"):
        R.global_registration_host(src, tgt[:20], **good)
    for field, value in (("voxel", 0.0), ("voxel", "x"), ("max_distance", -1.0), ("k", 64), ("iterations", 0), ("viewpoints", [(0, 0, 0)])):
        with pytest.raises(ValueError, match=field if field != "viewpoints" else "viewpoints"):
            R.check_global_settings(R.GlobalSettings(**{**dict(voxel=0.05), field: value}), 3)


def test_the_global_numpy_stream_is_not_touched():
    from randlanet.utils import registration as R
    src, tgt, _ = gi.planted("rot40-small")
    np.random.seed(11)
    want = np.random.uniform(size=4)
    np.random.seed(11)
    R.global_registration_host(src, tgt, max_distance=0.05, iterations=64)
    assert np.array_equal(np.random.uniform(size=4), want)


# ------------------------------------------------------------------------------------------------------ (e) planted cases
@pytest.mark.parametrize("name", tuple(gi.PLANTED))
def test_planted_motions_are_found_and_icp_finishes_them(name):
    from randlanet.utils import registration as R
    src, tgt, M = gi.planted(name)
    res = gi.planted_twin(name)
    rot, tr = ri.pose_error(res.transformation, M)
    print(f"{name}: global estimate {rot:.4f} degrees, {tr:.5f}; {res.count} inliers of {src.shape[0]}, status {res.status}")
    assert res.status == "refined" and rot < gi.GLOBAL_ROTATION_CAP and tr < gi.GLOBAL_TRANSLATION_CAP
    fine = R.icp_host(src, tgt, max_distance=gi.MAX_DISTANCE, init=res.transformation)
    rot, tr = ri.pose_error(fine.transformation, M)
    print(f"{name}: after icp {rot:.3e} degrees, {tr:.3e} (measured {gi.MEASURED_FINAL[name]})")
    assert rot < gi.FINAL_ROTATION_BOUND and tr < gi.FINAL_TRANSLATION_BOUND
    alone = R.icp_host(src, tgt, max_distance=gi.MAX_DISTANCE)                   # what the feature is needed for
    assert ri.pose_error(alone.transformation, M)[0] > 10.0


# --------------------------------------------------------------------------------------------------- (f) Model.predict_views
@pytest.fixture(scope="module")
def cpu_model():
    import torch
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    return Model(RandLANetSettings(n_classes=4, n_points=512, n_neighbors=8, layer_sizes=[8, 16, 32, 32]), use_gpu=False)


@pytest.mark.parametrize("to", ("first", "previous"))
def test_predict_views_with_global_init_on_a_cpu_placed_model(cpu_model, to):
    from randlanet.utils import registration as R
    views, motions = gi.views()
    vps = np.array([ri.moved_back(gi.VIEWPOINT[None], M)[0] for M in motions])
    model = cpu_model
    icp = R.IcpSettings(max_distance=0.05)
    settings = R.GlobalSettings(voxel=0.04, iterations=4096, viewpoints=tuple(map(tuple, vps)))
    want, poses = gi.views_by_hand(model, views, icp, settings, to, "cpu", vps)
    np.random.seed(5)
    got, found = model.predict_views(views, icp=icp, to=to, global_init=settings, return_global=True, **ri.KW)
    assert found[0] is None and all(np.array_equal(found[v].transformation, poses[v]) for v in (1, 2))
    for g, w in zip(got.confidences, want.confidences):
        assert np.array_equal(ri.bits(g), ri.bits(w))
    assert np.array_equal(ri.bits(got.transformations), ri.bits(want.transformations)) and got.status == want.status
    assert np.array_equal(ri.bits(got.xyz), ri.bits(want.xyz)) and np.array_equal(got.fitness, want.fitness)
    # the views are different samples of the surface, about 0.03 apart, so the pose is not exact: asked for is what
    # test_registration_cpu.py asks of ICP from a good start - under a degree, and a third of the samples' spacing
    for v in (1, 2):
        rot, tr = ri.pose_error(got.transformations[v], motions[v])
        print(f"view {v}: {rot:.4f} degrees, {tr:.5f}")
        assert rot < 1.0 and tr < 0.01, (v, rot, tr)
    np.random.seed(5)
    plain = model.predict_views(views, icp=icp, to=to, **ri.KW)                 # without it, ICP from the identity is lost
    assert ri.pose_error(plain.transformations[1], motions[1])[0] > 10.0
    np.random.seed(5)
    given = model.predict_views(views, icp=icp, to=to, poses=motions, global_init=settings, return_global=True, **ri.KW)
    assert given[1] == [None, None, None]                                       # views with a pose are untouched

