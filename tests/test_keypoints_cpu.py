"""Keypoints on the host: the numpy twin (utils/keypoints.py) against the brute-force definition of tests/keypoints_inputs.py on
every case, the properties of the definition, KeypointEvaluator on hand-worked examples, annotation_keypoints, and
Model.predict_keypoints on a CPU-placed model against the three steps - votes, labels, peaks - run on its own votes."""
import numpy as np
import pytest
import torch

import keypoints_inputs as ki

F32 = np.float32


# ------------------------------------------------------------------------------------------- 1. twin against brute force
@pytest.mark.parametrize("name", ki.CASES)
def test_twin_equals_brute_force(name):
    """index, classes, score and count are equal.  The twin adds the members' float64 terms in sorted-cell order, the brute
    force in index order - the same n = count terms.  With u = 2^-53: a sum of n terms is off by at most n u times the sum of
    their magnitudes, which for S_a is at most r W (|x_j - x_p| <= r, W the sum of the scores), so S_a / W is off by at most
    n u r from S_a and by at most n u |S_a / W| <= n u r from W: 2 n u r per order, n 2^-51 r between the two, inside
    count * 2^-50 * r with the roundings of the division and of x_p + S / W; then one rounding to float32, which can turn
    that into one spacing."""
    got, want = ki.twin(name), ki.brute(name)
    r = ki.case(name)[3]
    for f in ("index", "classes", "score", "count"):
        assert getattr(got, f).dtype == want[f].dtype == ki.DTYPES[f] and np.array_equal(getattr(got, f), want[f]), (name, f)
    assert got.position.dtype == F32 and got.position.shape == want["position"].shape == (got.index.shape[0], 3)
    bound = np.spacing(np.abs(want["position"])) + got.count[:, None].astype(np.float64) * 2.0 ** -50 * r
    err = np.abs(got.position.astype(np.float64) - want["position"].astype(np.float64))
    assert (err <= bound).all(), (name, float(err.max()))
    assert got.mean_score.dtype == F32 and got.mean_score.shape == got.index.shape
    assert (np.abs(got.mean_score.astype(np.float64) - want["mean_score"]) <= np.spacing(want["mean_score"])).all(), name


def test_what_the_cases_are_there_for():
    t = ki.twin
    xyz = ki.case("single")[0]
    assert t("single").index.tolist() == [0] and np.array_equal(t("single").position, xyz) and t("single").count.tolist() == [1]
    assert t("pair_at_r").index.tolist() == [1] and t("pair_at_r").count.tolist() == [2]
    assert t("pair_beyond_r").index.tolist() == [0, 1] and t("pair_beyond_r").count.tolist() == [1, 1]
    assert t("equal_scores_pair").index.tolist() == [0]
    for M in (4096, 4097):
        res = t(f"plateau_{M}")
        assert res.index.tolist() == [0] and res.count.tolist() == [M] and res.mean_score.tolist() == [0.5]
    dup = t("duplicates")                      # a coordinate's copies have one score: the first copy is the peak
    assert (dup.index < 40).all() and dup.count.min() >= 2
    assert t("neighbour_cells_26").index.tolist() == list(range(1, 52, 2))          # every stronger point, no weaker one
    assert (t("neighbour_cells_26").count == 2).all()
    xyz, lab, sc, r, kw = ki.case("flat")
    assert np.unique(xyz[:, 2]).size == 1 and t("flat").index.size > 10
    xyz, lab, sc, r, kw = ki.case("corner")
    from randlanet.utils import cluster as K
    o, dims = K.cluster_geometry(xyz, K.cell_edge(F32(r)))
    cells = np.floor((t("corner").position - o) / K.cell_edge(F32(r))).astype(np.int64)
    corners = {tuple(c) for c in cells.tolist()} & {(x, y, z) for x in (0, dims[0] - 1) for y in (0, dims[1] - 1)
                                                     for z in (0, dims[2] - 1)}
    assert len(corners) == 8
    # a stronger point of another class within r does not suppress: class by class the same keypoints
    xyz, lab, sc, r, kw = ki.case("touching_classes")
    from randlanet.utils.keypoints import confidence_peaks_host
    alone = [confidence_peaks_host(xyz, np.where(lab == c, lab, 0), sc, radius=r).index for c in (1, 2)]
    assert np.array_equal(np.sort(np.concatenate(alone)), t("touching_classes").index) and min(a.size for a in alone) > 3
    xyz, lab, sc, r, kw = ki.case("wide_labels")
    folded = confidence_peaks_host(xyz, lab & 0xffffffff, sc, radius=r)
    assert folded.index.size < t("wide_labels").index.size and (t("wide_labels").classes > 1 << 32).any()
    # the outlier (point 40, score 1.0) is not live at min_points 3; at 1 it is the peak and suppresses point 0
    assert t("lone_outlier").index.tolist() == [0] and t("lone_outlier").count.tolist() == [40]
    xyz, lab, sc, r, kw = ki.case("lone_outlier")
    loose = confidence_peaks_host(xyz, lab, sc, radius=r, min_points=1)
    assert 40 in loose.index and 0 not in loose.index
    zero = t("zero_scores")
    assert zero.index.size > 10 and np.array_equal(zero.position, ki.case("zero_scores")[0][zero.index])
    assert not zero.mean_score.any() and not zero.score.any()
    assert min(t(n).index.size for n in ("uniform_2049", "uniform_4097", "uniform_20000")) > 50


def test_empty_result_shapes_and_dtypes():
    res = ki.twin("nothing")
    assert res._fields == ki.FIELDS and type(res).__name__ == "KeypointResult"
    for f in ki.FIELDS:
        a = getattr(res, f)
        assert a.dtype == ki.DTYPES[f] and a.shape == ((0, 3) if f == "position" else (0,)), f
    # taking part but never live
    xyz, lab, sc, r, kw = ki.case("uniform_2049")
    from randlanet.utils.keypoints import confidence_peaks_host
    res = confidence_peaks_host(xyz, lab, sc, radius=r, min_points=3000)
    assert res.index.shape == (0,) and res.position.shape == (0, 3) and res.count.dtype == np.int32


# ------------------------------------------------------------------------------------------------------ 2. properties
@pytest.mark.parametrize("name", ["lattice_r", "duplicates", "uniform_4097", "uniform_20000", "flat"])
def test_peaks_of_a_label_are_more_than_r_apart_and_supported(name):
    """Supported: the participating points of its label within r of a keypoint, itself included, number min_points or more.
    `count` is the number of its members, the LIVE ones among those - at least the peak itself, at most the support - and
    may lie below min_points where a peak's neighbours are themselves short of support."""
    xyz, lab, sc, r, kw = ki.case(name)
    res = ki.twin(name)
    part = (lab >= 0) & ~np.isin(lab, kw.get("ignore_classes", (0,))) & (sc >= F32(kw.get("min_score", 0.0)))
    support = ki._near_rows(xyz, lab, part, F32(r) * F32(r), res.index).sum(axis=1)
    assert part[res.index].all() and (support >= kw.get("min_points", 1)).all()
    assert (res.count >= 1).all() and (res.count <= support).all()
    assert np.array_equal(res.index, np.sort(res.index)) and np.unique(res.index).size == res.index.size
    assert np.array_equal(res.classes, lab[res.index]) and np.array_equal(res.score, sc[res.index])
    p = xyz[res.index]
    d = p[:, None, :] - p[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == F32
    close = (d2 <= F32(r) * F32(r)) & (res.classes[:, None] == res.classes[None, :])
    assert np.array_equal(close, np.eye(res.index.size, dtype=bool))
    assert (np.abs(res.position - p) <= F32(r)).all()


def test_a_permutation_of_the_input_permutes_the_peaks():
    """With distinct scores the peaks do not depend on the order of the points."""
    from randlanet.utils.keypoints import confidence_peaks_host
    xyz, lab, _, r, kw = ki.case("uniform_4097")
    rs = np.random.RandomState(3)
    sc = (rs.permutation(xyz.shape[0]) / F32(8192)).astype(F32)                     # distinct, exact
    a = confidence_peaks_host(xyz, lab, sc, radius=r, **kw)
    perm = rs.permutation(xyz.shape[0])
    b = confidence_peaks_host(xyz[perm], lab[perm], sc[perm], radius=r, **kw)
    assert a.index.size > 50 and np.array_equal(np.sort(perm[b.index]), a.index)
    order = np.argsort(perm[b.index])
    assert np.array_equal(b.count[order], a.count) and np.array_equal(b.score[order], a.score)


def test_public_entry_on_the_cpu_is_the_twin_and_refuses():
    from randlanet.utils.keypoints import confidence_peaks
    xyz, lab, sc, r, kw = ki.case("uniform_2049")
    ki.assert_same(confidence_peaks(xyz, lab, sc, radius=r, device="cpu", **kw), ki.twin("uniform_2049"))
    ki.assert_same(confidence_peaks(xyz.astype(np.float64), lab.astype(np.int32), sc.astype(np.float64), radius=r,
                                    device="cpu", **kw), ki.twin("uniform_2049"))
    for bad, match in ((dict(radius=0.0), "radius"), (dict(radius=r, min_points=0), "min_points"),
                       (dict(radius=r, min_score=float("nan")), "min_score")):
        with pytest.raises(ValueError, match=match):
            confidence_peaks(xyz, lab, sc, device="cpu", **bad)
    for s in (None, sc[:-1], np.where(np.arange(sc.size) == 5, -0.5, sc), np.where(np.arange(sc.size) == 5, np.inf, sc)):
        with pytest.raises(ValueError, match="scores"):
            confidence_peaks(xyz, lab, s, radius=r, device="cpu")
    with pytest.raises(ValueError, match="labels"):
        confidence_peaks(xyz, lab.astype(F32), sc, radius=r, device="cpu")
    txyz, tlab, tsc = ki.too_fine()
    with pytest.raises(ValueError, match=r"reach 2\^16 = 65536 cells on an axis"):
        confidence_peaks(txyz, tlab, tsc, radius=1.0, device="cpu")
    assert confidence_peaks(txyz, tlab, tsc, radius=1.1, device="cpu").index.tolist() == [0, 1, 2]


# ------------------------------------------------------------------------------------------------------- 3. evaluator
def _ev(**kw):
    from randlanet.utils.keypoint_metrics import KeypointEvaluator
    return KeypointEvaluator(3, (0.1, 0.5), **kw)


GT = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float64)


def test_evaluator_perfect_set():
    ev = _ev()
    ev.add(GT + [0.0, 0.0, 0.05], [1, 1, 2], [0.9, 0.8, 0.7], GT, [1, 1, 2])
    out = ev.result()
    for d in ("0.1", "0.5"):
        for col in ("precision", "recall", "F1", "AP"):
            assert out[f"{col}@{d}"] == 1.0 and out[f"class 1 {col}@{d}"] == 1.0 and out[f"class 2 {col}@{d}"] == 1.0
            assert np.isnan(out[f"class 0 {col}@{d}"])                               # ignored
        assert abs(out[f"distance@{d}"] - 0.05) < 1e-12
    assert out["class 1 n_gt"] == 2 and out["class 1 n_pred"] == 2 and out["class 0 n_gt"] == 0


def test_evaluator_one_miss():
    ev = _ev()
    ev.add(GT[:1], [1], [0.9], GT[:2], None)                                         # without classes: class 1
    out = ev.result(["bg", "tip", "knuckle"])
    assert out["tip precision@0.1"] == 1.0 and out["tip recall@0.1"] == 0.5 and abs(out["tip F1@0.1"] - 2 / 3) < 1e-12
    assert out["tip AP@0.1"] == 0.5 and out["tip distance@0.1"] == 0.0
    assert np.isnan(out["knuckle recall@0.1"]) and np.isnan(out["knuckle precision@0.1"])
    assert out["recall@0.1"] == 0.5                                                  # the mean skips NaN


def test_evaluator_duplicate_is_a_false_positive_and_order_is_by_score():
    ev = _ev()
    # predictions 0 and 2 fall on ground truth 0: the stronger one (0.9, listed last) takes it at 0.02, the other one is a
    # false positive at both distances (ground truth 1 is 0.96 away); prediction 1 reaches ground truth 1, 0.45 away, at 0.5
    ev.add([[0.04, 0, 0], [0.55, 0, 0], [0.0, 0.02, 0]], [1, 1, 1], [0.6, 0.5, 0.9], GT[:2], [1, 1])
    out = ev.result()
    assert out["class 1 precision@0.1"] == 1 / 3 and out["class 1 recall@0.1"] == 0.5
    assert abs(out["class 1 distance@0.1"] - 0.02) < 1e-12
    assert out["class 1 AP@0.1"] == 0.5                      # TP, FP, FP: precision 1 at recall 0.5, nothing beyond
    assert out["class 1 precision@0.5"] == 2 / 3 and out["class 1 recall@0.5"] == 1.0
    # in order of score: TP, FP, TP - precision 1 up to recall 0.5, 2/3 up to recall 1
    assert abs(out["class 1 AP@0.5"] - (0.5 * 1.0 + 0.5 * 2 / 3)) < 1e-12
    assert abs(out["class 1 distance@0.5"] - (0.02 + 0.45) / 2) < 1e-12


def test_evaluator_wrong_class_empty_scene_and_ties():
    ev = _ev()
    ev.add(GT[:1], [2], [0.9], GT[:1], [1])                  # the right place, the wrong class
    ev.add(np.empty((0, 3)), np.empty(0, np.int64), np.empty(0), np.empty((0, 3)), None)        # an empty scene
    out = ev.result()
    assert out["class 1 recall@0.5"] == 0.0 and np.isnan(out["class 1 precision@0.5"]) and out["class 1 AP@0.5"] == 0.0
    assert out["class 2 precision@0.5"] == 0.0 and np.isnan(out["class 2 recall@0.5"]) and np.isnan(out["class 2 AP@0.5"])
    assert np.isnan(out["class 1 F1@0.5"]) and np.isnan(out["distance@0.5"]) and ev.scenes == 2
    # equal distances go to the lowest ground-truth index; equal scores are ordered by scene, then by keypoint number
    ev = _ev()
    ev.add([[0.5, 0, 0]], [1], [0.5], [[0.25, 0, 0], [0.75, 0, 0]], None)
    assert [r[3] for r in ev.rows[(1, 0.5)]] == [True] and ev.n_gt[1] == 2
    ev.add([[9, 9, 9], [0.25, 0, 0]], [1, 1], [0.5, 0.5], [[0.25, 0, 0]], None)
    rows = sorted(ev.rows[(1, 0.5)], key=lambda r: (-r[0], r[1], r[2]))
    assert [(r[1], r[2], r[3]) for r in rows] == [(0, 0, True), (1, 0, False), (1, 1, True)]
    with pytest.raises(ValueError, match="distances"):
        from randlanet.utils.keypoint_metrics import KeypointEvaluator
        KeypointEvaluator(3, ())
    with pytest.raises(ValueError, match="pred_classes"):
        ev.add(GT, [1, 1], [0.5, 0.5, 0.5], GT, None)


# --------------------------------------------------------------------------------------------------------- 4. helpers
def test_annotation_keypoints_both_modes():
    from randlanet.utils.keypoints import annotation_keypoints
    rs = np.random.RandomState(1)
    xyz = rs.uniform(0, 10, (500, 3)).astype(F32)
    clicks = np.array([[2, 2, 2], [2.5, 2, 2], [8, 8, 8]], F32)
    xyz[[10, 200, 499]] = clicks
    mask = np.zeros(500, np.int64)
    mask[[10, 200, 499]] = 1
    got = annotation_keypoints(xyz, mask)
    assert got.dtype == F32 and np.array_equal(got, clicks)
    # broadened into balls of radius 0.2, as a loader does: one keypoint per ball, at the centroid of its points
    ball = (np.linalg.norm(xyz[:, None, :] - clicks[None, :, :], axis=2) <= 0.2).any(axis=1)
    dense = np.concatenate([xyz, clicks[0] + rs.uniform(-0.1, 0.1, (20, 3)).astype(F32)])
    ball = np.concatenate([ball, np.ones(20, bool)])
    got = annotation_keypoints(dense, ball, radius=0.3)
    assert got.shape == (3, 3) and got.dtype == F32
    first = np.flatnonzero(ball & (np.linalg.norm(dense - clicks[0], axis=1) <= 0.2))
    assert first.size > 10 and np.allclose(got[0], dense[first].astype(np.float64).mean(axis=0), atol=1e-6)
    assert np.array_equal(got[1:], clicks[1:])
    assert annotation_keypoints(xyz, np.zeros(500, bool), radius=0.3).shape == (0, 3)
    with pytest.raises(ValueError, match="annotation"):
        annotation_keypoints(xyz, mask[:-1])


# --------------------------------------------------------------------------------------------------- 5. CPU-placed model
@pytest.fixture(scope="module")
def cpu_model():
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    return Model(RandLANetSettings(n_classes=4, n_points=2048, n_neighbors=8, layer_sizes=[16, 32]), use_gpu=False)


@pytest.mark.parametrize("grid", [None, 0.3])
def test_predict_keypoints_on_a_cpu_model_is_the_three_steps(cpu_model, grid):
    from randlanet._scene_path import VoteOptions
    from randlanet.utils import cluster as K
    from randlanet.utils.keypoints import confidence_peaks_host
    rs = np.random.RandomState(7)
    M = 5000
    xyz = rs.uniform(0, 6, (M, 3)).astype(F32)
    np.random.seed(5)
    opt = VoteOptions(votes=1, batch_size=2, smooth=0.95, seed=2, grid=grid)
    prob, _, inv, V, cloud, *_ = cpu_model._scene_path.vote(xyz, None, opt, device_out=False)
    label, conf = K.scene_labels(prob)
    # an untrained network is nowhere sure: the threshold is the median confidence, so that half of the points take part
    kw = dict(radius=0.45, min_score=float(np.median(conf)), min_points=2, ignore_classes=(0,))
    np.random.seed(5)
    got = cpu_model.predict_keypoints(xyz, votes=1, batch_size=2, seed=2, grid=grid, **kw)
    want = confidence_peaks_host(cloud[:, :3], label, conf, **kw)
    if grid is not None:
        assert 2048 < V < M
        first = np.array([np.flatnonzero(inv == v)[0] for v in want.index], np.int64).reshape(-1)
        assert (inv[first] == want.index).all()
        want = want._replace(index=first)
    else:
        assert inv is None and V == M
    ki.assert_same(got, want, f"grid={grid}")
    assert type(got).__name__ == "KeypointResult" and got.index.size >= 1
    assert (got.classes != 0).all() and (got.score >= F32(kw["min_score"])).all() and (got.count >= 1).all()


def test_predict_keypoints_refuses_before_it_votes_and_evaluate_is_the_evaluator(cpu_model):
    from randlanet.utils.keypoint_metrics import KeypointEvaluator
    xyz = np.random.RandomState(0).uniform(0, 5, (3000, 3)).astype(F32)
    state = np.random.get_state()[1].copy()
    for bad, match in ((dict(radius=0.0), "radius"), (dict(radius=0.5, min_points=0), "min_points"),
                       (dict(radius=0.5, min_score=float("nan")), "min_score")):
        with pytest.raises(ValueError, match=match):
            cpu_model.predict_keypoints(xyz, **bad)
    nan = xyz.copy()
    nan[5, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        cpu_model.predict_keypoints(nan, radius=0.5)
    with pytest.raises(ValueError, match="scene 0"):
        cpu_model.evaluate_keypoints([(xyz, None)], radius=0.5)
    assert np.array_equal(np.random.get_state()[1], state)       # no forward ran: no permutation was drawn
    kw = dict(radius=0.5, min_score=0.0, ignore_classes=(), votes=1, batch_size=2, seed=2)
    gt = xyz[::500]
    np.random.seed(5)
    got = cpu_model.evaluate_keypoints([(xyz, None, gt)], distances=(0.25, 1.0), **kw)
    np.random.seed(5)
    res = cpu_model.predict_keypoints(xyz, **kw)
    ev = KeypointEvaluator(4, (0.25, 1.0), ignore_classes=())
    ev.add(res.position, res.classes, res.score, gt, None)
    want = ev.result()
    assert list(got) == list(want) and all(got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])) for k in got)
    assert "AP@0.25" in got and "class 1 distance@1" in got and res.index.size > 10


# --------------------------------------------------------------------------------------------------------- 6. C ABI
def test_new_entries_are_exported_and_check_their_arguments_on_the_host():
    from randlanet import _hip
    for n in ("rl_keypoints_workspace_bytes", "rl_keypoints_cells", "rl_keypoints_sort", "rl_keypoints_support",
              "rl_keypoints_peaks", "rl_keypoints_refine"):
        assert n in _hip.EXPORTS
    lib = _hip.lib()
    M = 5000
    need = lib.rl_keypoints_workspace_bytes(M)
    assert need > 52 * M and need % 256 == 0
    assert lib.rl_keypoints_workspace_bytes(0) == 0 and lib.rl_keypoints_workspace_bytes(2 ** 31 - 1) == 0
    assert all(lib.rl_keypoints_workspace_bytes(m) % 256 == 0 for m in (1, 63, 2049, 10 ** 7, 2 ** 31 - 2))
    fake = 1 << 20              # never dereferenced: every call below is refused before a launch
    E = _hip.ERR_ARGS
    assert lib.rl_keypoints_cells(fake, M, 0.0, fake, fake, need, None) == E
    assert b"rl_keypoints_cells: radius=0 must be positive and finite" in lib.rl_last_error()
    assert lib.rl_keypoints_cells(fake, M, 0.5, fake, fake, need - 1, None) == E
    assert b"workspace" in lib.rl_last_error()
    assert lib.rl_keypoints_cells(fake, M, 0.5, fake, fake + 8, need, None) == E
    assert b"aligned" in lib.rl_last_error()
    assert lib.rl_keypoints_sort(fake, fake, fake, M, float("nan"), None, 0, 10, fake, need, None) == E
    assert b"min_score" in lib.rl_last_error()
    assert lib.rl_keypoints_sort(fake, fake, fake, M, 0.0, None, 1, 10, fake, need, None) == E
    assert b"ignored classes" in lib.rl_last_error()
    assert lib.rl_keypoints_sort(fake, fake, fake, M, 0.0, None, 0, 50, fake, need, None) == E
    assert b"key_bits=50" in lib.rl_last_error()
    assert lib.rl_keypoints_sort(fake, fake, None, M, 0.0, None, 0, 10, fake, need, None) == E
    assert lib.rl_keypoints_support(fake, M, -1.0, fake, need, None) == E
    assert lib.rl_keypoints_support(None, M, 0.5, fake, need, None) == E
    assert lib.rl_keypoints_peaks(fake, M, 0.5, 0, fake, fake, need, None) == E
    assert b"min_points=0" in lib.rl_last_error()
    assert lib.rl_keypoints_peaks(fake, 0, 0.5, 1, fake, fake, need, None) == E
    out = (fake,) * 6
    assert lib.rl_keypoints_refine(fake, M, 0, 0.5, 1, *out, fake, need, None) == E
    assert b"K=0 keypoints" in lib.rl_last_error()
    assert lib.rl_keypoints_refine(fake, M, M + 1, 0.5, 1, *out, fake, need, None) == E
    assert lib.rl_keypoints_refine(fake, M, 3, 0.5, 1, fake, fake, None, fake, fake, fake, fake, need, None) == E
    assert b"null pointer" in lib.rl_last_error()
