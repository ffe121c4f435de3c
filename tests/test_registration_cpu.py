"""Rigid registration (utils/registration.py) without a GPU: the numpy twin recovers a planted motion, one evaluation agrees
with an independent float64 restatement, the counts and correspondences are exact, every refusal names its argument, and a
CPU-placed Model's predict_views equals the same steps done by hand."""
import numpy as np
import pytest

import registration_inputs as ri

F32 = np.float32


# ------------------------------------------------------------------------------------------------ (a) the planted motion
@pytest.mark.parametrize("metric", ri.METRICS)
@pytest.mark.parametrize("max_distance", (0.1, 0.05))
def test_twin_recovers_the_planted_motion(metric, max_distance):
    """1500 points of a 3000-point room corner, moved by the inverse of 5 degrees about (1, 2, 2) / 3 plus (0.03, -0.02,
    0.01).  Measured with this twin on the CPU, over the two gates: point_to_plane 4 updates, rotation error <= 3.2e-7
    degrees, translation error <= 4.8e-9, rmse <= 5.0e-8; point_to_point 8 updates, rotation error <= 2.4e-7 degrees,
    translation error <= 1.5e-8, rmse <= 5.1e-8.  The residual is the float32 rounding of coordinates of extent 1 (2^-24 =
    6e-8 per coordinate); the bounds are 10x the larger measured value of each quantity."""
    res = ri.twin(f"planted-{metric}-{max_distance}")
    rot, tr = ri.pose_error(res.transformation, ri.motion())
    print(metric, max_distance, res.status, res.updates, res.fitness, res.inlier_rmse, rot, tr)
    assert res.status == "converged" and res.fitness == 1.0 and res.count == 1500
    assert 1 <= res.updates <= 30 and res.history.shape == (res.updates + 1, 30)
    assert rot <= 3.2e-6 and tr <= 1.5e-7 and res.inlier_rmse <= 5.1e-7
    assert (res.correspondence >= 0).all() and res.transformed.dtype == F32


# ------------------------------------------------------------------------------ (b) one evaluation, restated in float64
def _nearest(tgt, q):
    """The K-NN contract by numpy: un-fused float32 d2, the first minimum."""
    idx, d2 = np.empty(q.shape[0], np.int64), np.empty(q.shape[0], F32)
    for i, p in enumerate(q):
        d = tgt - p
        s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        idx[i] = int(np.argmin(s))
        d2[i] = s[idx[i]]
    return idx, d2


def _jacobians(p, n):
    return np.concatenate([np.cross(p, n), n], axis=1)


@pytest.mark.parametrize("metric", ri.METRICS)
def test_one_evaluation_against_a_float64_restatement(metric):
    from randlanet.utils import registration as R
    from randlanet.utils.normals import estimate_normals_host
    src, tgt, _ = ri.case(f"{metric}-1025-3000")
    T = ri.motion(1.5, 0.5 * ri.SHIFT)
    got = R.evaluate_registration(src, tgt, T, 0.004, metric=metric, device="cpu")
    assert got.status == "iterations" and got.updates == 0 and got.history.shape == (1, 30)
    assert np.array_equal(got.transformation, T)
    # the transform is the stated float32 expression
    R32, t32 = T[:3, :3].astype(F32), T[:3, 3].astype(F32)
    q = np.stack([F32(F32(F32(R32[a, 0] * src[:, 0]) + F32(R32[a, 1] * src[:, 1])) + F32(R32[a, 2] * src[:, 2])) + t32[a]
                  for a in range(3)], axis=1)
    assert q.dtype == F32 and np.array_equal(ri.bits(got.transformed), ri.bits(q))
    assert np.array_equal(ri.bits(R.apply_transform(src, T, device="cpu")), ri.bits(q))
    # count and correspondence are exact
    idx, d2 = _nearest(tgt, q)
    g2 = F32(0.004) * F32(0.004)
    valid = d2 <= g2
    assert 100 < valid.sum() < 1000                                 # the gate cuts through the cloud
    assert got.count == valid.sum() == int(got.history[0, 0]) and got.fitness == valid.sum() / 1025
    assert np.array_equal(got.correspondence, np.where(valid, idx, -1))
    # A, b, the residual and the distance sum against J.T @ J and J.T @ r
    p, y = q[valid].astype(np.float64), tgt[idx[valid]].astype(np.float64)
    if metric == "point_to_plane":
        normals = [estimate_normals_host(tgt, 16).normals[idx[valid]].astype(np.float64)]
    else:
        normals = [np.broadcast_to(e, p.shape) for e in np.eye(3)]
    J = np.concatenate([_jacobians(p, n) for n in normals])
    r = np.concatenate([((p - y) * n).sum(axis=1) for n in normals])
    A, b = R.normal_equations(got.history[0])
    eps = 29 * 2.0 ** -53
    assert (np.abs(A - J.T @ J) <= eps * (np.abs(J).T @ np.abs(J))).all()
    assert (np.abs(b - J.T @ r) <= eps * (np.abs(J).T @ np.abs(r))).all()
    assert abs(got.history[0, 28] - r @ r) <= eps * (r @ r)
    D = d2[valid].astype(np.float64).sum()
    assert abs(got.history[0, 29] - D) <= eps * D and got.inlier_rmse == np.sqrt(got.history[0, 29] / got.count)
    assert (np.abs(A) > 0).sum() >= 24 and (b != 0).all()          # (the comparison is not one of zeros)


# ------------------------------------------------------------------------------------------------------- (c) the rest
def test_zero_iterations_is_evaluate_registration():
    from randlanet.utils import registration as R
    src, tgt, kw = ri.case("planted-point_to_plane-0.1")
    T = ri.motion(4.0)
    a = R.icp_host(src, tgt, max_distance=0.1, iterations=0, init=T)
    b = R.evaluate_registration(src, tgt, T, 0.1, device="cpu")
    c = R.icp(src, tgt, max_distance=0.1, iterations=0, init=T, device="cpu")
    ri.assert_same(a, b)
    ri.assert_same(a, c)
    assert a.status == "iterations" and a.updates == 0
    first = ri.twin("planted-point_to_plane-0.1")
    again = R.evaluate_registration(src, tgt, first.transformation, 0.1, device="cpu")
    assert np.array_equal(again.history[0], first.history[-1]) and np.array_equal(again.transformed, first.transformed)
    assert again.fitness == first.fitness and again.inlier_rmse == first.inlier_rmse


def test_degenerate_cases():
    from randlanet.utils import registration as R
    res = ri.twin("gated_out")
    assert res.status == "degenerate" and res.updates == 0 and res.count == 0 and res.fitness == 0.0 and res.inlier_rmse == 0.0
    assert (res.correspondence == -1).all() and not res.history.any() and np.array_equal(res.transformation, np.eye(4))
    one = ri.twin("one_pair")
    assert one.status == "degenerate" and one.count == 1 and np.flatnonzero(one.correspondence >= 0).tolist() == [1030]
    assert one.correspondence[1030] == 17
    # a planar target under point to plane: three columns of J are exactly zero, the factorisation meets a zero pivot and
    # np.linalg.solve raises - "degenerate", nothing moved
    rs = np.random.RandomState(3)
    tgt = np.concatenate([rs.uniform(0, 1, (500, 2)), np.zeros((500, 1))], axis=1).astype(F32)
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], F32), (500, 1))
    src = tgt[:200] + np.array([0.01, 0.0, 0.02], F32)
    res = R.icp_host(src, tgt, max_distance=0.2, target_normals=nrm)
    A, b = R.normal_equations(res.history[0])
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.solve(A, -b)
    assert res.status == "degenerate" and res.updates == 0 and res.count == 200 and R.step(res.history[0]) is None
    # fewer pairs than min_pairs
    few = R.icp_host(src[:5], tgt, max_distance=0.2, metric="point_to_point")
    assert few.status == "degenerate" and few.count == 5
    assert R.icp_host(src[:5], tgt, max_distance=0.2, metric="point_to_point", min_pairs=3).updates >= 1


def test_the_sign_of_a_normal_does_not_matter():
    from randlanet.utils import registration as R
    from randlanet.utils.normals import estimate_normals_host
    src, tgt, kw = ri.case("planted-point_to_plane-0.1")
    nrm = estimate_normals_host(tgt, 16).normals
    a = R.icp_host(src, tgt, target_normals=nrm, **kw)
    flip = np.where((np.arange(3000) % 2 == 0)[:, None], -nrm, nrm)
    ri.assert_same(R.icp_host(src, tgt, target_normals=flip, **kw), a)
    ri.assert_same(a, ri.twin("planted-point_to_plane-0.1"))       # the default normals are estimate_normals(target, 16)
    zero = ri.twin("zero_normals")
    assert zero.count == 1000 and zero.fitness == 1.0              # a zero normal still counts as a pair


def test_ties_go_to_the_lowest_index():
    res = ri.twin("duplicates")
    assert res.count == 500 and (res.correspondence < 1000).all() and (res.correspondence >= 0).all()


def test_history_and_settings():
    from randlanet.utils import registration as R
    res = ri.twin("planted-point_to_point-0.05")
    assert res.history.shape == (res.updates + 1, 30) and (res.history[:, 0] <= 1500).all()
    A, _ = R.normal_equations(res.history[0])
    assert np.array_equal(A, A.T) and A[3, 3] == A[4, 4] == A[5, 5] == res.history[0, 0]       # sum of e_a . e_a = count
    capped = R.icp_host(*ri.case("planted-point_to_point-0.05")[:2], max_distance=0.05, metric="point_to_point", iterations=2)
    assert capped.status == "iterations" and capped.updates == 2
    assert np.array_equal(capped.history, res.history[:3])
    s = R.IcpSettings(0.05)
    assert (s.metric, s.normals, s.iterations, s.min_pairs) == ("point_to_plane", 16, 30, 6)
    with pytest.raises(Exception):
        s.metric = "x"


def test_every_refusal_names_its_argument():
    from randlanet.utils import registration as R
    src, tgt, _ = ri.case("point_to_plane-63-300")
    ok = dict(max_distance=0.1)
    bad_T = np.eye(4)
    bad_T[0, 0] = 2.0
    nan = np.array(src)
    nan[5, 1] = np.nan
    for fn in (R.icp_host, lambda *a, **k: R.icp(*a, device="cpu", **k)):
        for kw, match in ((dict(max_distance=0.0), "max_distance"), (dict(max_distance=float("nan")), "max_distance"),
                          (dict(max_distance=-1.0), "max_distance"), (dict(max_distance=1e30), "max_distance"),
                          (dict(max_distance="x"), "max_distance"),
                          (dict(ok, metric="plane"), "metric"), (dict(ok, iterations=-1), "iterations"),
                          (dict(ok, iterations=257), "iterations"), (dict(ok, iterations=2.5), "iterations"),
                          (dict(ok, normals=2), "normals"), (dict(ok, normals=65), "normals"),
                          (dict(ok, init=np.eye(3)), "init"), (dict(ok, init=bad_T), "init"),
                          (dict(ok, relative_fitness=-1e-3), "relative_fitness"),
                          (dict(ok, relative_rmse=float("inf")), "relative_rmse"), (dict(ok, min_pairs=0), "min_pairs"),
                          (dict(ok, target_normals=np.zeros((299, 3), F32)), "target_normals")):
            with pytest.raises(ValueError, match=match):
                fn(src, tgt, **kw)
        for s, t, match in ((src[:, :2], tgt, "source"), (src, tgt.reshape(-1), "target"), (nan, tgt, "source"),
                            (src, np.zeros((0, 3), F32), "target"), (np.zeros((0, 3), F32), tgt, "source")):
            with pytest.raises(ValueError, match=match):
                fn(s, t, **ok)
        with pytest.raises(ValueError, match="fewer than normals=16"):
            fn(src, tgt[:10], **ok)
        assert fn(src, tgt[:10], metric="point_to_point", **ok).count >= 0       # no normals needed
    with pytest.raises(ValueError, match="apply_transform: T"):
        R.apply_transform(src, bad_T, device="cpu")
    with pytest.raises(ValueError, match="xyz"):
        R.apply_transform(src[:, :2], np.eye(4), device="cpu")


def test_c_abi_entries_refuse_without_a_gpu():
    from randlanet import _hip as H
    lib = H.lib()
    for n in ("rl_icp_workspace_bytes", "rl_icp_transform", "rl_icp_sums", "rl_icp_fold"):
        assert n in H.EXPORTS
    for Ms in (-1, 0, 2 ** 31 - 1, 2 ** 40):
        assert lib.rl_icp_workspace_bytes(Ms) == 0
    for Ms in (1, 1024, 1025, 66561, 10 ** 6, 2 ** 31 - 2):
        chunks = -(-Ms // 1024)
        n = lib.rl_icp_workspace_bytes(Ms)
        assert n % 256 == 0 and 236 * chunks <= n <= 236 * chunks + 512
    before = lib.rl_launch_count()
    assert lib.rl_icp_transform(None, 10, 0, 10, None, None, None) == H.ERR_ARGS
    assert lib.rl_icp_sums(None, None, None, 10, None, None, 10, 0, 10, 1.0, 0, None, None, 0, None) == H.ERR_ARGS
    assert lib.rl_icp_fold(10, None, None, 0, None) == H.ERR_ARGS
    assert lib.rl_launch_count() == before


# ------------------------------------------------------------------------------------------------------- (d) the Model
@pytest.fixture(scope="module")
def cpu_model():
    import torch
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    return Model(RandLANetSettings(n_classes=4, n_points=512, n_neighbors=8, layer_sizes=[8, 16, 32, 32]), use_gpu=False)


KW = ri.KW


@pytest.mark.parametrize("to", ("first", "previous"))
def test_predict_views_equals_the_composition_by_hand(cpu_model, to):
    from randlanet.utils.registration import IcpSettings
    views = ri.views3()
    settings = IcpSettings(0.08, iterations=10)
    np.random.seed(5)
    got = cpu_model.predict_views(views, icp=settings, to=to, **KW)
    want, T, xyz = ri.by_hand(cpu_model, views, settings, to, "cpu")
    assert np.array_equal(ri.bits(got.transformations), ri.bits(T)) and np.array_equal(ri.bits(got.xyz), ri.bits(xyz))
    assert [c.shape for c in got.confidences] == [(4, 700), (4, 600), (4, 500)]
    assert np.array_equal(ri.bits(np.concatenate(got.confidences, axis=1)), ri.bits(want))
    assert got.status[0] == "reference" and all(s in ("converged", "iterations") for s in got.status[1:])
    assert got.fitness.shape == (3,) and got.fitness[0] == 1.0 and (got.fitness[1:] > 0.9).all() and got.inlier_rmse[0] == 0.0
    # the views came back to the corner's frame.  They are different samples of the surface, about 0.03 apart, so the pose
    # is not exact: asked for is a quarter of the planted angle and a third of the samples' spacing
    for v, deg, f in ((1, 2.0, 0.3), (2, 3.0, 0.5)):
        rot, tr = ri.pose_error(got.transformations[v], ri.motion(deg, f * ri.SHIFT))
        assert rot < deg / 4 and tr < 0.01, (v, rot, tr)


def test_predict_views_refusals_and_poses(cpu_model):
    from randlanet.utils.registration import IcpSettings
    views = ri.views3()
    s = IcpSettings(0.08, iterations=10)
    with pytest.raises(ValueError, match="IcpSettings"):
        cpu_model.predict_views(views, icp=dict(max_distance=0.1))
    with pytest.raises(ValueError, match="to="):
        cpu_model.predict_views(views, icp=s, to="last")
    with pytest.raises(ValueError, match="poses"):
        cpu_model.predict_views(views, icp=s, poses=[None])
    with pytest.raises(ValueError, match=r"poses\[1\]"):
        cpu_model.predict_views(views, icp=s, poses=[None, np.zeros((4, 4)), None])
    with pytest.raises(ValueError, match="return_counts"):
        cpu_model.predict_views(views, icp=s, return_counts=True)
    with pytest.raises(ValueError, match=r"views\[2\]"):
        cpu_model.predict_views(views[:2] + [np.zeros((0, 3), F32)], icp=s)
    with pytest.raises(ValueError, match="max_distance"):
        cpu_model.predict_views(views, icp=IcpSettings(-1.0))
    with pytest.raises(ValueError, match="all of one kind"):
        cpu_model.predict_views([views[0], (views[1], np.zeros((600, 2), F32))], icp=s)
    # a pose that is already right: the registration has nothing left to do but confirm it
    np.random.seed(5)
    got = cpu_model.predict_views(views[:2], icp=s, poses=[None, ri.motion(2.0, 0.3 * ri.SHIFT)], **KW)
    np.random.seed(5)
    plain = cpu_model.predict_views(views[:2], icp=s, **KW)
    assert got.status[1] == "converged" and ri.pose_error(got.transformations[1], plain.transformations[1])[0] < 0.05
