"""Smoothness-constrained clustering without a GPU: the numpy twin (utils/cluster.py with normals and normal_angle) against
the brute-force definition of tests/smooth_inputs.py on every case, what the cases are there for, the refusals, normals=None
against the plain functions, Model.predict_instances(normal_angle=...) on a CPU-placed model, and the C ABI of the new
entries."""
import numpy as np
import pytest
import torch

import cluster_inputs as ci
import smooth_inputs as sm
from smooth_twin import twin

F32 = np.float32


# ------------------------------------------------------------------------------------------- 1. twin == the definition
@pytest.mark.parametrize("name", sm.CASES)
def test_twin_equals_brute_force(name):
    res, want = twin(name), sm.brute(name)
    sm.assert_same(res, want, name)
    M = sm.case(name)[0].shape[0]
    assert res.instance.shape == (M,) and res.instance.dtype == np.int32
    I = res.count.shape[0]
    assert res.instance.max(initial=-1) == I - 1
    assert np.array_equal(np.bincount(res.instance[res.instance >= 0], minlength=I), res.count)


@pytest.mark.parametrize("name", ci.CASES)
def test_all_normals_equal_is_the_plain_rule(name):
    """The smooth twin with every normal (0, 0, 1) against the plain twin: every edge case of distance, cells and numbering."""
    sm.assert_same(twin("equal:" + name), ci.twin(name), name)


def test_what_the_cases_are_there_for():
    """The expected shape of the answer, from the brute force: a case that no longer holds its edge shows here."""
    b = sm.brute
    # the behaviour the feature exists for: a floor and a wall that share an edge
    assert b("corner_plain")["count"].tolist() == [1800]
    assert sorted(b("corner")["count"].tolist()) == [900, 900]
    xyz, _, _, kw = sm.case("corner")
    inst = b("corner")["instance"]
    floor = kw["normals"][:, 2] == 1
    assert floor.sum() == 900 and len(set(inst[floor])) == 1 and len(set(inst[~floor])) == 1
    # exactly at the threshold: joined; one float32 step below: not
    _, _, _, kw = sm.case("threshold")
    n = kw["normals"]
    assert (n[0, 0] * n[1, 0] + n[0, 1] * n[1, 1]) + n[0, 2] * n[1, 2] == sm.cos_of(30.0)
    assert (n[2, 0] * n[3, 0] + n[2, 1] * n[3, 1]) + n[2, 2] * n[3, 2] == np.nextafter(sm.cos_of(30.0), F32(0))
    assert b("threshold")["instance"].tolist() == [0, 0, 1, 2]
    # the sign of a normal does not matter
    assert (sm.case("flipped")[3]["normals"][:, 2] == -1).sum() == 200
    assert b("flipped")["count"].tolist() == [400]
    # a zero normal joins nobody, at 89 degrees either
    z = b("zero_normals")["count"]
    assert sorted(z.tolist()) == [1] * 15 + [105, 105]
    # transitivity carries a component around a bend; below the step between neighbours nothing is joined
    assert b("ring_10")["count"].tolist() == [72]
    assert b("ring_3")["count"].tolist() == [1] * 72
    # the blended normals of the crease bridge the two surfaces at 80 degrees; cutting them by curvature separates them
    assert b("crease_bridges")["count"].tolist() == [1800]
    cut = b("crease_cut")
    xyz, _, _, kw = sm.case("crease_cut")
    high = kw["curvature"] > 0.1
    assert high.sum() == 90 and (cut["instance"][high] == -1).all() and (cut["instance"][~high] >= 0).all()
    assert sorted(cut["count"].tolist()) == [840, 870]
    # dense contention: components of more than one size, at least one of 100 points or more
    one = b("dense:one_cell_4096")["count"]
    assert sorted(one.tolist()) == [301, 3795]
    u = b("dense:uniform_20000")["count"]
    assert u.shape == (2423,) and len(set(u.tolist())) == 51 and int(u.max()) == 3347 and int((u >= 5).sum()) == 240
    assert b("dense:uniform_20000_min5")["count"].shape == (240,)
    assert 1 not in b("dense:uniform_20000")["classes"]
    c = b("curv:uniform_4097")
    _, lab, _, kw = sm.case("curv:uniform_4097")
    assert c["count"].shape == (1119,) and int(c["count"].max()) == 24
    assert int(((lab > 0) & (kw["curvature"] > F32(0.2))).sum()) == 1024
    assert (c["instance"][kw["curvature"] > F32(0.2)] == -1).all()
    # the smooth rule cut the dense clouds: the plain rule finds one component, and 5361 points in the largest
    assert ci.brute("one_cell_4096")["count"].tolist() == [4096] and int(ci.brute("uniform_20000")["count"].max()) == 5361


def test_the_directions_of_the_dense_cases():
    d = sm.DIRECTIONS.astype(np.float64)
    assert d.shape == (12, 3) and np.allclose(np.linalg.norm(d, axis=1), 1, atol=1e-6)
    ang = np.degrees(np.arccos(np.clip(np.abs(d @ d.T), 0, 1)))
    agree = ang <= 40
    assert np.abs(ang[~np.eye(12, dtype=bool)] - 40).min() > 0.4          # no pair near the threshold
    assert agree[:11, :11].sum() == 115 and not agree[0, 10] and not agree[11, :11].any()


# ------------------------------------------------------------------------------------------------------ 2. refusals
def test_refusals():
    from randlanet.utils.cluster import euclidean_clusters, euclidean_clusters_host
    xyz = np.random.RandomState(1).uniform(0, 1, (10, 3)).astype(F32)
    lab = np.ones(10, np.int64)
    nrm = np.tile(np.array([0, 0, 1], F32), (10, 1))
    curv = np.zeros(10, F32)
    for fn in (euclidean_clusters_host, lambda *a, **k: euclidean_clusters(*a, device="cpu", **k)):
        with pytest.raises(ValueError, match="normals and normal_angle go together"):
            fn(xyz, lab, radius=0.1, normals=nrm)
        with pytest.raises(ValueError, match="normals and normal_angle go together"):
            fn(xyz, lab, radius=0.1, normal_angle=30)
        with pytest.raises(ValueError, match="curvature and max_curvature go together"):
            fn(xyz, lab, radius=0.1, normals=nrm, normal_angle=30, curvature=curv)
        with pytest.raises(ValueError, match="curvature and max_curvature go together"):
            fn(xyz, lab, radius=0.1, normals=nrm, normal_angle=30, max_curvature=0.1)
        with pytest.raises(ValueError, match="need normals and normal_angle"):
            fn(xyz, lab, radius=0.1, curvature=curv, max_curvature=0.1)
        with pytest.raises(ValueError, match="need normals and normal_angle"):
            fn(xyz, lab, radius=0.1, max_curvature=0.1)
        for bad in (0, 90, -5, 120, np.nan, np.inf, "wide", (30, 40)):
            with pytest.raises(ValueError, match=r"normal_angle=.* must be a number of degrees in \(0, 90\)"):
                fn(xyz, lab, radius=0.1, normals=nrm, normal_angle=bad)
        with pytest.raises(ValueError, match=r"normals have shape \(10, 2\)"):
            fn(xyz, lab, radius=0.1, normals=nrm[:, :2], normal_angle=30)
        with pytest.raises(ValueError, match=r"normals have shape \(9, 3\)"):
            fn(xyz, lab, radius=0.1, normals=nrm[:9], normal_angle=30)
        for bad in (np.nan, np.inf, -np.inf, 1e40):
            n = nrm.astype(np.float64)
            n[6, 1] = bad
            with pytest.raises(ValueError, match="non-finite normals, first at point 6"):
                fn(xyz, lab, radius=0.1, normals=n, normal_angle=30)
        with pytest.raises(ValueError, match=r"curvature has shape \(10, 1\)"):
            fn(xyz, lab, radius=0.1, normals=nrm, normal_angle=30, curvature=curv[:, None], max_curvature=0.1)
        for bad in (np.nan, np.inf):
            c = curv.copy()
            c[3] = bad
            with pytest.raises(ValueError, match="non-finite curvature, first at point 3"):
                fn(xyz, lab, radius=0.1, normals=nrm, normal_angle=30, curvature=c, max_curvature=0.1)
        for bad in (np.nan, "high", (0.1, 0.2)):
            with pytest.raises(ValueError, match="max_curvature=.* must be a number, not NaN"):
                fn(xyz, lab, radius=0.1, normals=nrm, normal_angle=30, curvature=curv, max_curvature=bad)
        # the plain refusals still come first, and an infinite max_curvature is a number: nothing is cut
        with pytest.raises(ValueError, match="must be positive and finite"):
            fn(xyz, lab, radius=0.0, normals=nrm, normal_angle=30)
        res = fn(xyz, lab, radius=2.0, normals=nrm, normal_angle=30, curvature=curv + 5, max_curvature=np.inf)
        assert res.count.tolist() == [10]
        res = fn(xyz, lab, radius=2.0, normals=nrm, normal_angle=30, curvature=curv, max_curvature=-np.inf)
        assert res.count.shape == (0,) and (res.instance == -1).all()
        # the curvature equal to the maximum still takes part: only a greater one is cut
        c = curv.copy()
        c[:4] = F32(0.1)
        c[4] = np.nextafter(F32(0.1), F32(1))
        res = fn(xyz, lab, radius=2.0, normals=nrm, normal_angle=30, curvature=c, max_curvature=0.1)
        assert res.count.tolist() == [9] and res.instance[4] == -1


def test_without_normals_nothing_changes():
    from randlanet.utils import cluster as K
    for name in ("uniform_257", "lattice_r", "touching_classes"):
        xyz, lab, r, kw = ci.case(name)
        for fn in (K.euclidean_clusters_host, lambda *a, **k: K.euclidean_clusters(*a, device="cpu", **k)):
            res = fn(xyz, lab, radius=r, scores=ci.scores_of(name), normals=None, normal_angle=None, curvature=None,
                     max_curvature=None, **kw)
            ci.assert_same(res, ci.brute(name), name)
    # check_inputs keeps its six arguments and its six results; takes_part its two
    out = K.check_inputs(np.zeros((2, 3)), np.zeros(2, np.int64), 0.5, 1, (0,), None)
    assert len(out) == 6
    assert K.takes_part(np.array([0, 1, -1, 2]), np.array([0])).tolist() == [False, True, False, True]
    assert K.check_smooth(5, None, None) is None


def test_the_threshold_is_the_float32_cosine():
    from randlanet.utils import cluster as K
    for angle in (1e-3, 10, 30.0, 45, np.float32(60), 89.999):
        _, cos_t, curv, top = K.check_smooth(1, np.zeros((1, 3)), angle)
        assert cos_t.dtype == F32 and cos_t == sm.cos_of(angle) and 0 < cos_t <= 1 and curv is None and top is None
    nrm, _, curv, top = K.check_smooth(2, [[0, 0, 1], [1, 0, 0]], 30, np.array([0.5, 1.0]), 0.1)
    assert nrm.dtype == F32 and nrm.flags.c_contiguous and curv.dtype == F32 and top == F32(0.1) and top.dtype == F32


# --------------------------------------------------------------------------------------------------- 3. CPU-placed model
def _cpu_model(n_features):
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    return Model(RandLANetSettings(n_classes=4, n_points=1024, n_neighbors=8, layer_sizes=[8, 16, 32, 32],
                                   n_features=n_features), use_gpu=False)


def _room(rs, M):
    """A floor and two walls that meet in creases, sampled at random, with a little noise."""
    xyz = rs.uniform(0, 4, (M, 3))
    face = rs.randint(0, 3, M)
    xyz[np.arange(M), (2 - face)] = 0.0
    return (xyz + rs.normal(0, 0.003, (M, 3))).astype(F32)


@pytest.mark.parametrize("mode", ["appended", "estimated", "estimated_grid_curvature"])
def test_predict_instances_on_a_cpu_model_is_the_steps(mode):
    from randlanet._scene_path import VoteOptions
    from randlanet.utils import cluster as K
    from randlanet.utils import grid as G
    from randlanet.utils import normals as NU
    model = _cpu_model(4 if mode == "appended" else 0)
    rs = np.random.RandomState(7)
    M = 3000
    xyz = _room(rs, M)
    vp = (2.0, 2.0, 2.0)
    kw = dict(votes=1, batch_size=2, seed=2, viewpoint=vp)
    radius, min_points, ignore, min_conf, angle = 0.3, 2, (3,), 0.0, 6.0
    smooth = dict(normal_angle=angle)
    k = 16
    if mode == "appended":
        kw["normals"] = k
    else:
        k = smooth["cluster_normals"] = 12
    cloud, inverse = xyz, None
    if mode == "estimated_grid_curvature":
        kw["grid"] = 0.12
        smooth["max_curvature"] = 0.02
        sub = G.grid_subsample_host(xyz, cell=0.12)
        cloud, inverse = sub.xyz, sub.inverse
        assert 1024 < cloud.shape[0] < M
    np.random.seed(5)
    got = model.predict_instances(xyz, radius=radius, min_points=min_points, ignore_classes=ignore,
                                  min_confidence=min_conf, **kw, **smooth)
    np.random.seed(5)
    opt = VoteOptions(votes=1, batch_size=2, smooth=0.95, seed=2, grid=kw.get("grid"), normals=kw.get("normals"), viewpoint=vp)
    prob, _, inv, V, voted, *_ = model._scene_path.vote(xyz, None, opt, device_out=False)
    assert V == cloud.shape[0] and np.array_equal(voted[:, :3], cloud)
    label, conf = K.scene_labels(prob, min_conf)
    est = NU.estimate_normals_host(cloud, k, vp)
    if mode == "appended":                              # the columns the network saw are the twin's
        assert voted.shape[1] == 7 and np.array_equal(voted[:, 3:6], est.normals)
        assert np.array_equal(voted[:, 6], est.curvature)
    else:
        assert voted.shape[1] == 3
    extra = dict(curvature=est.curvature, max_curvature=smooth["max_curvature"]) if "max_curvature" in smooth else {}
    want = K.euclidean_clusters_host(cloud, label, radius=radius, min_points=min_points, ignore_classes=ignore, scores=conf,
                                     normals=est.normals, normal_angle=angle, **extra)
    plain = K.euclidean_clusters_host(cloud, label, radius=radius, min_points=min_points, ignore_classes=ignore, scores=conf)
    if inverse is not None:
        assert np.array_equal(inv, inverse)
        label, want = label[inverse], want._replace(instance=want.instance[inverse])
    assert np.array_equal(got.label, label)
    ci.assert_same(got, want, mode)
    # the rule did something on this scene: the answer differs from the plain one
    assert want.count.shape[0] >= 1 and not np.array_equal(want.count, plain.count)
    if extra:
        cut = (est.curvature > F32(0.02))
        assert cut.any() and (want.instance[np.isin(inverse, np.flatnonzero(cut))] == -1).all()
    # normal_angle=None is the plain path
    np.random.seed(5)
    got = model.predict_instances(xyz, radius=radius, min_points=min_points, ignore_classes=ignore,
                                  min_confidence=min_conf, **kw)
    if inverse is not None:
        plain = plain._replace(instance=plain.instance[inverse])
    ci.assert_same(got, plain, mode + " plain")


def test_predict_instances_refuses_before_it_votes():
    model = _cpu_model(0)
    xyz = np.random.RandomState(0).uniform(0, 5, (2000, 3)).astype(F32)
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError, match="max_curvature needs normal_angle"):
        model.predict_instances(xyz, radius=0.5, max_curvature=0.1)
    with pytest.raises(ValueError, match="normal_angle=95"):
        model.predict_instances(xyz, radius=0.5, normal_angle=95)
    with pytest.raises(ValueError, match="max_curvature=nan"):
        model.predict_instances(xyz, radius=0.5, normal_angle=30, max_curvature=float("nan"))
    with pytest.raises(ValueError, match="k=2 must be an integer in 3 .. 64"):
        model.predict_instances(xyz, radius=0.5, normal_angle=30, cluster_normals=2)
    with pytest.raises(ValueError, match="viewpoint"):
        model.predict_instances(xyz, radius=0.5, normal_angle=30, viewpoint=(1, 2))
    with pytest.raises(ValueError, match="max_curvature needs normal_angle"):
        model.evaluate_instances([(xyz, None, np.zeros(2000, np.int64), np.zeros(2000, np.int64))], radius=0.5,
                                 max_curvature=0.1)
    assert np.array_equal(np.random.get_state()[1], state)       # no forward ran: no permutation was drawn
    # a cloud of fewer points than cluster_normals: the error of normals=k
    with pytest.raises(ValueError, match="the scene has 40 points, fewer than the normals=k=48 neighbours of a normal"):
        model.predict_instances(xyz[:40], radius=0.5, normal_angle=30, cluster_normals=48, pad_small_scenes=True)


# --------------------------------------------------------------------------------------------------------- 4. C ABI
def test_new_entries_are_exported_and_check_their_arguments_on_the_host():
    from randlanet import _hip
    for n in ("rl_cluster_smooth_workspace_bytes", "rl_cluster_union_smooth"):
        assert n in _hip.EXPORTS
    lib = _hip.lib()
    M = 5000
    plain, need = lib.rl_cluster_workspace_bytes(M), lib.rl_cluster_smooth_workspace_bytes(M)
    assert need == plain + 16 * M + (-16 * M) % 256          # the plain layout as its prefix, then a float4 per point
    assert lib.rl_cluster_smooth_workspace_bytes(0) == 0 and lib.rl_cluster_smooth_workspace_bytes(2 ** 31 - 1) == 0
    fake = 1 << 20              # never dereferenced: every call below is refused before a launch
    E = _hip.ERR_ARGS

    def union(M=M, radius=0.5, ignore=None, n_ignore=0, key_bits=10, min_points=1, normals=fake, curvature=None, cos=0.9,
              top=0.0, ws=fake, ws_bytes=need, xyz=fake):
        return lib.rl_cluster_union_smooth(xyz, fake, M, radius, ignore, n_ignore, key_bits, min_points, normals, curvature,
                                           cos, top, fake, fake, ws, ws_bytes, None)
    assert union(normals=None) == E and b"rl_cluster_union_smooth: null pointer" in lib.rl_last_error()
    assert union(xyz=None) == E
    for bad in (0.0, -0.5, 1.5, float("nan")):
        assert union(cos=bad) == E and b"cos_angle" in lib.rl_last_error()
    assert union(curvature=fake, top=float("nan")) == E and b"max_curvature is not a number" in lib.rl_last_error()
    assert union(ws_bytes=plain) == E and b"workspace" in lib.rl_last_error()       # the plain workspace is too small
    assert union(ws_bytes=need - 1) == E
    assert union(ws=fake + 8) == E and b"aligned" in lib.rl_last_error()
    assert union(min_points=0) == E and b"rl_cluster_union_smooth: min_points=0" in lib.rl_last_error()
    assert union(n_ignore=1) == E and b"ignored classes" in lib.rl_last_error()
    assert union(key_bits=50) == E and b"key_bits=50" in lib.rl_last_error()
    assert union(radius=-1.0) == E and union(M=0) == E
    # the shared calls accept the larger workspace
    assert lib.rl_cluster_cells(None, M, 0.5, fake, fake, need, None) == E and b"null pointer" in lib.rl_last_error()
