"""Instance evaluation without a GPU: the numpy twin of the pair counts (utils/instance_metrics.py) against a dense brute
force on the cases of tests/pairs_inputs.py, its refusals, the C ABI of the rl_pairs_* entries, the scoring protocol on cases
worked by hand, and Model.evaluate_instances on a CPU-placed model against predict_instances + InstanceEvaluator by hand."""
import math

import numpy as np
import pytest
import torch

import pairs_inputs as pi

F32 = np.float32


def same_result(got, want):
    assert list(got.keys()) == list(want.keys())
    for k in got:
        g, w = got[k], want[k]
        assert (g == w) or (isinstance(g, float) and math.isnan(g) and math.isnan(w)), (k, g, w)


# ------------------------------------------------------------------------------------------------- 1. twin == brute force
@pytest.mark.parametrize("name", pi.SMALL)
def test_twin_equals_the_dense_table(name):
    pa, pb, n = pi.twin(name)
    wa, wb, wn = pi.brute(name)
    assert pa.dtype == np.int32 and pb.dtype == np.int32 and n.dtype == np.int64
    assert np.array_equal(pa, wa) and np.array_equal(pb, wb) and np.array_equal(n, wn)
    assert n.sum() == pi.case(name)[0].shape[0] and (n > 0).all()
    key = (pa.astype(np.int64) + 1) * (pi.case(name)[3] + 1) + pb + 1
    assert (np.diff(key) > 0).all()                                  # ascending (a, b), -1 first, every pair once


def test_what_the_cases_are_there_for():
    from randlanet.utils.instance_metrics import key_bits
    for name, bits in pi.WIDTHS.items():
        _, _, A, B = pi.case(name)
        assert key_bits(A, B) == bits, name
    assert (key_bits(1 << 20, 1 << 20) + 7) // 8 == 6 and (key_bits(65535, 65536) + 7) // 8 == 5
    assert pi.twin("all_equal")[2].tolist() == [5000] and pi.twin("all_distinct")[2].tolist() == [1] * 5000
    assert [x.tolist() for x in pi.twin("all_minus_one")] == [[-1], [-1], [4099]]
    assert pi.case("below_minus_one")[0].min() == -5 and pi.twin("below_minus_one")[0].min() == -1
    assert pi.twin("bit0")[0].tolist() == [-1, -1] and pi.twin("bit0")[1].tolist() == [-1, 0]
    runs = pi.twin("long_runs")[2]
    assert (runs[:-1] == 3000).all() and 3000 % pi.CHUNK != 0 and runs.shape[0] == 24
    a, _, _, B = pi.case("bits_37_high_only")
    keys = np.unique((a + 1) * (B + 1) + 6)
    assert keys.size == 16 and ((keys ^ keys[0]) & ((1 << 32) - 1) == 0).all()      # they differ above bit 32 only
    pa, pb, _ = pi.twin("bits_41")
    assert pa.max() == (1 << 20) - 1 and pb.max() == (1 << 20) - 1 and pa.shape[0] > 1000
    assert pi.case("int32_70001")[0].dtype == np.int32 and pi.case("mixed_dtypes")[1].dtype == np.int16


# ------------------------------------------------------------------------------------------------------- 2. refusals
def test_refusals():
    from randlanet.utils.instance_metrics import pair_counts, pair_counts_host
    a = np.array([0, 1, 2, -1, -7]), np.array([1, 0, 0, 0, -1])
    for fn in (pair_counts_host, lambda *x: pair_counts(*x, device="cpu")):
        assert [r.tolist() for r in fn(a[0], a[1], 3, 2)] == [[-1, -1, 0, 1, 2], [-1, 0, 1, 0, 0], [1, 1, 1, 1, 1]]
        with pytest.raises(ValueError, match="out of range"):
            fn(a[0], a[1], 2, 2)                                     # a value == A
        with pytest.raises(ValueError, match="out of range"):
            fn(a[0], a[1], 3, 1)
        with pytest.raises(ValueError, match="out of range"):
            fn(a[0].astype(np.uint64), a[1], 3, 2)                  # -1 as uint64 is 2^64 - 1
        with pytest.raises(ValueError, match=r"exceeds 2\^62"):
            fn(a[0], a[1], 1 << 31, 1 << 31)
        with pytest.raises(ValueError, match="int32"):
            fn(a[0], a[1], 1 << 31, 1)
        for bad in ((0, 2), (3, 0), (-1, 2), (2.5, 2)):
            with pytest.raises(ValueError, match="must be integers >= 1"):
                fn(a[0], a[1], *bad)
        with pytest.raises(ValueError, match=r"M=0 points"):
            fn(np.zeros(0, np.int64), np.zeros(0, np.int64), 3, 2)
        with pytest.raises(ValueError, match=r"b has shape \(4,\)"):
            fn(a[0], a[1][:4], 3, 2)
        with pytest.raises(ValueError, match=r"a has shape \(5, 1\)"):
            fn(a[0][:, None], a[1], 3, 2)
        with pytest.raises(ValueError, match="dtype float64"):
            fn(a[0].astype(np.float64), a[1], 3, 2)
    # the largest sizes that are accepted
    assert pair_counts_host(a[0], a[1], (1 << 31) - 1, (1 << 31) - 1)[2].sum() == 5


# ---------------------------------------------------------------------------------------------------------- 3. C ABI
def test_new_entries_are_exported_and_check_their_arguments_on_the_host():
    from randlanet import _hip
    for n in ("rl_pairs_workspace_bytes", "rl_pairs_sort", "rl_pairs_write"):
        assert n in _hip.EXPORTS
    lib = _hip.lib()
    M = 5000
    need = lib.rl_pairs_workspace_bytes(M)
    assert need > 28 * M and lib.rl_pairs_workspace_bytes(0) == 0 and lib.rl_pairs_workspace_bytes(2 ** 31 - 1) == 0
    assert lib.rl_pairs_workspace_bytes(2 ** 31 - 2) > 28 * (2 ** 31 - 2)
    fake = 1 << 20              # never dereferenced: every call below is refused before a launch
    E = _hip.ERR_ARGS
    ok = (fake, 4, fake, 8, M, 10, 10, fake, fake, need, None)

    def sort_with(**kw):
        names = ("a", "a_bytes", "b", "b_bytes", "M", "A", "B", "head", "ws", "ws_bytes", "stream")
        args = dict(zip(names, ok))
        args.update(kw)
        return lib.rl_pairs_sort(*(args[n] for n in names))

    assert sort_with(M=0) == E and b"rl_pairs_sort: M=0 outside" in lib.rl_last_error()
    assert sort_with(M=2 ** 31 - 1) == E
    assert sort_with(A=0) == E and b"A=0" in lib.rl_last_error()
    assert sort_with(B=2 ** 31) == E and b"B=2147483648" in lib.rl_last_error()
    assert sort_with(a_bytes=2) == E and b"int32 or int64" in lib.rl_last_error()
    assert sort_with(b_bytes=0) == E
    assert sort_with(ws_bytes=need - 1) == E and b"workspace" in lib.rl_last_error()
    assert sort_with(ws=fake + 8) == E and b"aligned" in lib.rl_last_error()
    assert sort_with(ws=None) == E and b"null pointer" in lib.rl_last_error()
    assert sort_with(a=None) == E and sort_with(b=None) == E and sort_with(head=None) == E
    assert b"rl_pairs_sort: null pointer" in lib.rl_last_error()

    okw = (M, 10, 10, 7, fake, fake, fake, fake, need, None)

    def write_with(**kw):
        names = ("M", "A", "B", "P", "pa", "pb", "count", "ws", "ws_bytes", "stream")
        args = dict(zip(names, okw))
        args.update(kw)
        return lib.rl_pairs_write(*(args[n] for n in names))

    assert write_with(P=0) == E and b"P=0 pairs" in lib.rl_last_error()
    assert write_with(P=M + 1) == E
    assert write_with(M=-1) == E and write_with(A=0) == E and write_with(B=0) == E
    assert write_with(ws_bytes=need - 1) == E and b"workspace" in lib.rl_last_error()
    assert write_with(ws=fake + 128) == E and b"aligned" in lib.rl_last_error()
    assert write_with(ws=None) == E
    assert write_with(pa=None) == E and write_with(pb=None) == E and write_with(count=None) == E
    assert b"rl_pairs_write: null pointer" in lib.rl_last_error()


# -------------------------------------------------------------------------------------------------- 4. the protocol by hand
def hand_scene(g_ids=(0, 1)):
    """24 points, one class of interest (1): g0 = points 0-9, g1 = 10-19, 20-23 unlabelled; p0 = 0-7 (0.9), p1 = 8-13 (0.8),
    p2 = 14-21 (0.7), p3 = 22-23 (0.95)."""
    gt = np.full(24, -1)
    gt[0:10], gt[10:20] = g_ids
    labels = np.where(gt >= 0, 1, 0)
    pred = np.empty(24, np.int32)
    pred[0:8], pred[8:14], pred[14:22], pred[22:24] = 0, 1, 2, 3
    return pred, np.array([1, 1, 1, 1]), np.array([0.9, 0.8, 0.7, 0.95], F32), gt, labels


def evaluator(n_classes=2, **kw):
    from randlanet.utils.instance_metrics import InstanceEvaluator
    kw.setdefault("device", "cpu")
    return InstanceEvaluator(n_classes, **kw)


def check_hand_result(r):
    assert r["AP25"] == 1.0 and r["AP50"] == 0.5 and r["AP"] == 0.3
    assert r["precision50"] == 1 / 3 and r["recall50"] == 0.5
    assert r["mCov"] == 0.65 and r["mWCov"] == 0.65
    assert r["class 1 AP25"] == 1.0 and r["class 1 AP50"] == 0.5 and r["class 1 AP"] == 0.3
    assert r["class 1 n_gt"] == 2 and r["class 1 n_pred"] == 4
    assert math.isnan(r["class 0 AP"]) and r["class 0 n_gt"] == 0 and r["class 0 n_pred"] == 0


def test_the_hand_case():
    ev = evaluator()
    assert ev.thresholds == (0.25, 0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95)
    ev.add(*hand_scene())
    # p3 (instance 3) is dropped at every threshold; the others are kept, in descending score
    for t in ev.thresholds:
        rows = ev.kept[(1, t)]
        assert [r[2] for r in rows] == [0, 1, 2]
        want = {0.25: [True, True, False], 0.5: [True, False, False]}.get(t, [t < 0.8, False, False])
        assert [r[3] for r in rows] == want, t
    r = ev.result()
    check_hand_result(r)
    # AP per threshold: 0.5 for 0.50 .. 0.75, 0 from 0.80 on (0.8 is not above 0.8)
    for t in ev.ap_thresholds:
        e = evaluator(iou_thresholds=(t,))
        e.add(*hand_scene())
        assert e.result()["AP"] == (0.5 if t < 0.8 else 0.0), t
    named = ev.result(class_names=["floor", "chair"])
    assert named["chair AP50"] == 0.5 and "class 1 AP50" not in named
    with pytest.raises(ValueError, match="class names"):
        ev.result(class_names=["chair"])


def test_non_dense_ground_truth_ids_and_unlabelled_points():
    ev = evaluator()
    ev.add(*hand_scene(g_ids=(5, 17)))                       # ids without points do not exist
    check_hand_result(ev.result())
    # unlabelled by the label instead of the instance id, by an ignored class, and by a label outside [0, n_classes)
    pred, pc, ps, gt, labels = hand_scene()
    gt2, labels2 = gt.copy(), labels.copy()
    gt2[20:24] = 9
    labels2[20:24] = [0, 0, 2, -1]
    ev = evaluator()
    ev.add(pred, pc, ps, gt2, labels2)
    check_hand_result(ev.result())
    # the class of a ground-truth instance is its most frequent label, ties to the lowest
    ev = evaluator(n_classes=3)
    labels3 = labels.copy()
    labels3[0:5] = 2                                         # g0: five points of class 1, five of class 2 -> class 1
    labels3[10:14] = 2                                       # g1: six of class 1, four of class 2 -> class 1
    ev.add(pred, pc, ps, gt, labels3)
    r = ev.result()
    assert r["class 1 n_gt"] == 2 and r["class 2 n_gt"] == 0 and r["class 1 AP50"] == 0.5


def test_two_scenes_are_pooled_not_averaged():
    def scene_a(score):
        gt = np.full(12, -1)
        gt[:10] = 0
        return gt.copy(), np.array([1]), np.array([score]), gt, np.where(gt >= 0, 1, 0)

    def scene_b(score):
        gt = np.repeat([0, 1], 10)
        pred = np.full(20, -1)
        pred[0:5], pred[10:15], pred[15:20] = 0, 0, 1        # p0: IoU 5/15 with both; p1: IoU 5/10 with g1
        return pred, np.array([1, 1]), np.array([score, 0.3]), gt, np.ones(20, np.int64)

    ev = evaluator()
    ev.add(*scene_a(0.6))
    ev.add(*scene_b(0.9))
    r = ev.result()
    # at 0.5 over N_pos = 3: FP (0.9), TP (0.6), FP (0.3): one recall step of 1/3 at precision 1/2
    assert r["AP50"] == (1.0 / 3.0) * 0.5 and r["precision50"] == 1 / 3 and r["recall50"] == 1 / 3
    assert r["AP25"] == 1.0 and r["class 1 n_gt"] == 3 and r["class 1 n_pred"] == 3
    # coverage: 1, 1/3 and 1/2 over three instances of ten points
    assert r["mCov"] == (1.0 + 5 / 15 + 0.5) / 3 and r["mWCov"] == (10 * 1.0 + 10 * (5 / 15) + 10 * 0.5) / 30
    alone = []
    for sc in (scene_a(0.6), scene_b(0.9)):
        e = evaluator()
        e.add(*sc)
        alone.append(e.result()["AP50"])
    assert alone == [1.0, 0.0]
    # equal scores: the scene added first comes first
    for order, want in (((scene_a, scene_b), 1.0 / 3.0), ((scene_b, scene_a), (1.0 / 3.0) * 0.5)):
        e = evaluator()
        for sc in order:
            e.add(*sc(0.6))
        assert e.result()["AP50"] == want


def test_classes_without_predictions_and_without_ground_truth():
    pred, pc, ps, gt, labels = hand_scene()
    gt, labels = np.concatenate((gt, [2] * 6)), np.concatenate((labels, [2] * 6))         # an object of class 2, not predicted
    pred = np.concatenate((pred, [-1] * 6))
    ev = evaluator(n_classes=4)
    ev.add(pred, pc, ps, gt, labels)
    r = ev.result()
    assert r["class 2 AP"] == 0.0 and r["class 2 AP50"] == 0.0 and r["class 2 AP25"] == 0.0
    assert r["class 2 recall50"] == 0.0 and math.isnan(r["class 2 precision50"]) and r["class 2 Cov"] == 0.0
    assert r["class 2 n_gt"] == 1 and r["class 2 n_pred"] == 0
    for key in ("AP", "AP50", "AP25", "recall50", "Cov", "WCov"):
        assert math.isnan(r[f"class 3 {key}"]), key                 # no ground truth
    assert r["class 3 n_gt"] == 0
    # the means skip class 3 (and the ignored class 0), and class 2 without predictions in precision50
    assert r["AP50"] == (0.5 + 0.0) / 2 and r["AP25"] == 0.5 and r["AP"] == (0.3 + 0.0) / 2
    assert r["recall50"] == 0.25 and r["precision50"] == 1 / 3 and r["mCov"] == 0.65 / 2
    # a prediction of a class without ground truth changes no score of that class: it stays NaN
    ev = evaluator(n_classes=4)
    ev.add(pred, np.array([1, 1, 1, 3]), ps, gt, labels)
    r2 = ev.result()
    assert math.isnan(r2["class 3 AP50"]) and r2["class 3 n_pred"] == 1 and r2["AP50"] == r["AP50"]
    # nothing predicted at all
    ev = evaluator()
    ev.add(np.full(24, -1), np.zeros(0, np.int64), np.zeros(0, F32), *hand_scene()[3:])
    r = ev.result()
    assert r["AP"] == 0.0 and r["mCov"] == 0.0 and r["class 1 n_pred"] == 0 and r["class 1 n_gt"] == 2


def test_min_gt_points_drops_the_match_and_lowers_n_pos():
    gt = np.array([0] * 12 + [1] * 4 + [-1] * 2)
    labels = np.where(gt >= 0, 1, 0)
    pred = gt.copy()
    pred[16:18] = 2                                          # p2 lies in the void: dropped whatever min_gt_points is
    args = (pred, np.array([1, 1, 1]), np.array([0.9, 0.8, 0.7]), gt, labels)
    ev = evaluator(min_gt_points=4)
    ev.add(*args)
    r = ev.result()
    assert [row[2:] for row in ev.kept[(1, 0.5)]] == [(0, True), (1, True)]
    assert r["class 1 n_gt"] == 2 and r["AP50"] == 1.0 and r["recall50"] == 1.0 and r["mCov"] == 1.0
    ev = evaluator(min_gt_points=5)                          # g1 has four points: ignored
    ev.add(*args)
    r = ev.result()
    assert [row[2:] for row in ev.kept[(1, 0.5)]] == [(0, True)]             # p1 is dropped, not an FP
    assert r["class 1 n_gt"] == 1 and r["AP50"] == 1.0 and r["precision50"] == 1.0 and r["class 1 n_pred"] == 3
    # a prediction that only grazes the ignored instance is dropped through its void share
    pred2 = pred.copy()
    pred2[12:14] = -1                                        # p1 = two points of g1: IoU 0.5 with it, void share 1
    ev = evaluator(min_gt_points=5)
    ev.add(pred2, *args[1:])
    assert [row[2:] for row in ev.kept[(1, 0.5)]] == [(0, True)]
    ev = evaluator(min_gt_points=1)
    ev.add(pred2, *args[1:])
    assert [row[2:] for row in ev.kept[(1, 0.5)]] == [(0, True), (1, False)]     # 0.5 is not above 0.5: an FP
    assert [row[2:] for row in ev.kept[(1, 0.25)]] == [(0, True), (1, True)]


def test_evaluator_refusals():
    from randlanet.utils.instance_metrics import InstanceEvaluator
    pred, pc, ps, gt, labels = hand_scene()
    for kw in (dict(n_classes=0), dict(n_classes=2, min_gt_points=0), dict(n_classes=2, iou_thresholds=(1.0,)),
               dict(n_classes=2, iou_thresholds=())):
        with pytest.raises(ValueError):
            InstanceEvaluator(device="cpu", **kw)
    ev = evaluator()
    with pytest.raises(ValueError, match="gt_instance has shape"):
        ev.add(pred, pc, ps, gt.astype(np.float64), labels)
    with pytest.raises(ValueError, match="gt_labels have shape"):
        ev.add(pred, pc, ps, gt, labels[:5])
    with pytest.raises(ValueError, match="pred_instance has shape"):
        ev.add(pred[:5], pc, ps, gt, labels)
    with pytest.raises(ValueError, match="pred_scores have shape"):
        ev.add(pred, pc, ps[:3], gt, labels)
    with pytest.raises(ValueError, match="out of range"):
        ev.add(pred, pc[:3], ps[:3], gt, labels)             # instance 3 without a class
    with pytest.raises(ValueError, match="pred_classes is empty"):
        ev.add(np.zeros(24, np.int64), pc[:0], ps[:0], gt, labels)
    assert ev.scenes == 0


# --------------------------------------------------------------------------------------------------- 5. CPU-placed model
@pytest.fixture(scope="module")
def cpu_model():
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    return Model(RandLANetSettings(n_classes=4, n_points=1024, n_neighbors=8, layer_sizes=[8, 16, 32, 32]), use_gpu=False)


def model_scenes(sizes, seed=7):
    """Scenes in a 6 m box with 2 m columns as ground-truth objects (ids with gaps), class 1 + id % 3, a slab of class 0."""
    rs = np.random.RandomState(seed)
    scenes = []
    for M in sizes:
        xyz = rs.uniform(0, 6, (M, 3)).astype(F32)
        ids = (np.floor(xyz[:, 0] / 2) + 4 * np.floor(xyz[:, 1] / 2)).astype(np.int64)
        labels = 1 + ids % 3
        labels[xyz[:, 2] < 0.5] = 0
        ids[xyz[:, 2] > 5.8] = -1
        scenes.append((xyz, None, labels, ids))
    return scenes


@pytest.mark.parametrize("grid", [None, 0.3])
def test_evaluate_instances_on_a_cpu_model_is_the_steps_by_hand(cpu_model, grid):
    scenes = model_scenes((3000, 2500))
    kw = dict(radius=0.45, min_points=2, ignore_classes=(3,), min_confidence=0.26, votes=1, batch_size=2, seed=2, grid=grid)
    names = ["a", "b", "c", "d"]
    np.random.seed(5)
    got = cpu_model.evaluate_instances(scenes, names, min_gt_points=20, **kw)
    np.random.seed(5)
    ev = evaluator(n_classes=4, ignore_classes=(3,), min_gt_points=20)
    n_pred = 0
    for xyz, features, labels, ids in scenes:
        res = cpu_model.predict_instances(xyz, features, **kw)
        ev.add(res.instance, res.classes, res.score, ids, labels)
        n_pred += res.count.shape[0]
    same_result(got, ev.result(names))
    assert n_pred >= 1 and sum(got[f"{n} n_pred"] for n in names[:3]) == n_pred and got["d n_pred"] == 0
    assert got["a n_gt"] + got["b n_gt"] + got["c n_gt"] >= 9 and math.isnan(got["d AP"])
    assert 0.0 <= got["mCov"] <= 1.0 and 0.0 <= got["AP25"] <= 1.0


def test_evaluate_instances_refuses_before_it_votes(cpu_model):
    (xyz, _, labels, ids), = model_scenes((2000,))
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError, match="not a tuple"):
        cpu_model.evaluate_instances([(xyz, None, labels)], radius=0.5)
    with pytest.raises(ValueError, match="instance_ids have shape"):
        cpu_model.evaluate_instances([(xyz, None, labels, ids[:-1])], radius=0.5)
    with pytest.raises(ValueError, match="instance_ids have shape .* dtype float64"):
        cpu_model.evaluate_instances([(xyz, None, labels, ids.astype(np.float64))], radius=0.5)
    with pytest.raises(ValueError, match="labels have shape"):
        cpu_model.evaluate_instances([(xyz, None, labels[:, None], ids)], radius=0.5)
    with pytest.raises(ValueError, match="labels have shape .* dtype float32"):
        cpu_model.evaluate_instances([(xyz, None, labels.astype(F32), ids)], radius=0.5)
    with pytest.raises(ValueError, match="class names"):
        cpu_model.evaluate_instances([(xyz, None, labels, ids)], ["a", "b"], radius=0.5)
    # a bad second scene is found before the first one is voted on
    with pytest.raises(ValueError, match="scene 1"):
        cpu_model.evaluate_instances([(xyz, None, labels, ids), (xyz, None, labels)], radius=0.5)
    with pytest.raises(ValueError, match="radius"):
        cpu_model.evaluate_instances([(xyz, None, labels, ids)], radius=0.0)
    with pytest.raises(ValueError, match="min_gt_points"):
        cpu_model.evaluate_instances([(xyz, None, labels, ids)], radius=0.5, min_gt_points=0)
    assert np.array_equal(np.random.get_state()[1], state)       # no forward ran: no permutation was drawn
