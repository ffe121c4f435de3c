"""Oriented boxes without a GPU: the numpy twin of csrc/boxes.hip (utils/boxes.py) against an independent float64 oracle,
its structure, its degenerate ids and its refusals; the host-side argument checks of the rl_boxes_* entries; box AP
(utils/box_metrics.py) on scenes whose score is known by construction; Model.predict_instances(oriented_boxes=True) and
Model.evaluate_instances(boxes=True) on a CPU-placed model."""
import numpy as np
import pytest
import torch

import boxes_inputs as bi

F32 = np.float32
ULP64 = np.finfo(np.float64).eps


def _members(name):
    xyz, ids, n_ids = bi.case(name)
    I = bi.twin(name).count.shape[0]
    return [xyz[ids == k] for k in range(I)]


# ------------------------------------------------------------------------------------- 1. the twin against an oracle
def _oracle(P32):
    """Plain float64: mean, covariance, numpy's eigh, projection.  Returns (axes rows, longest first; extent), rounded once."""
    P = P32.astype(np.float64)
    mu = P.mean(axis=0)
    d = P - mu
    lam, V = np.linalg.eigh(d.T @ d / P.shape[0])
    axes = V[:, ::-1].T
    t = d @ axes.T
    return axes.astype(F32), (t.max(axis=0) - t.min(axis=0)).astype(F32)


@pytest.mark.parametrize("name", bi.ORACLE_CASES)
def test_twin_equals_an_independent_oracle(name):
    """Both sides do their work in float64 on the same float32 points and round once, so they may differ by a rounding
    boundary: extents within 2 float32 ulps at the largest extent of the case (tighter than ulps at coordinate + extent, which
    the contract allows up to 8 of), axes - up to sign - within 2 ulps at 1.  Measured on these cases: 0 ulp for both - every
    float32 of the twin equals the oracle's."""
    got = bi.twin(name)
    worst_e = worst_a = 0.0
    for k, P in enumerate(_members(name)):
        assert P.shape[0] >= 256
        axes, extent = _oracle(P)
        ulp_e = float(np.spacing(F32(got.extent.max())))
        e = np.abs(got.extent[k].astype(np.float64) - extent).max() / ulp_e
        sign = np.sign((got.axes[k].astype(np.float64) * axes).sum(axis=1))
        a = np.abs(got.axes[k].astype(np.float64) - sign[:, None] * axes).max() / float(np.spacing(F32(1)))
        worst_e, worst_a = max(worst_e, e), max(worst_a, a)
    print(f"{name}: extents within {worst_e} ulp, axes within {worst_a} ulp")
    assert worst_e <= 2 and worst_a <= 2


# ---------------------------------------------------------------------------------------------------- 2. structure
@pytest.mark.parametrize("name", bi.CASES)
def test_axes_are_orthonormal_and_right_handed_before_rounding(name):
    from randlanet.utils import boxes as B
    pts, ids, I = B.check_inputs(*bi.case(name))
    _, count, mean, cov = B.moments_host(pts, ids, I)
    axes, lam = B.axes_from_covariance(cov)
    gram = axes @ axes.transpose(0, 2, 1)
    worst = np.abs(gram - np.eye(3)).max(initial=0.0) / ULP64
    print(f"{name}: |A A^T - 1| <= {worst} fp64 ulp")
    assert worst <= 4
    assert np.abs(axes[:, 2] - np.cross(axes[:, 0], axes[:, 1])).max(initial=0.0) <= 4 * ULP64
    assert (np.linalg.det(axes) > 0.999999).all()
    assert (lam[:, 0] >= lam[:, 1]).all() and (lam[:, 1] >= lam[:, 2]).all()
    for a in range(2):                               # the component of largest magnitude is positive
        big = np.argmax(np.abs(axes[:, a]), axis=1)
        assert (axes[np.arange(I), a, big] > 0).all()


@pytest.mark.parametrize("name", bi.CASES)
def test_count_box_and_containment(name):
    res = bi.twin(name)
    xyz, ids, _ = bi.case(name)
    assert [a.dtype for a in res] == [np.int32] + [F32] * 6
    I = res.count.shape[0]
    assert res.axes.shape == (I, 3, 3) and all(a.shape == (I, 3) for a in (res.lo, res.hi, res.center, res.extent))
    scale = float(np.abs(xyz).max()) + float(res.extent.max(initial=0.0))
    tol = 4 * float(np.spacing(F32(scale)))
    for k, P in enumerate(_members(name)):
        assert res.count[k] == P.shape[0]
        if P.shape[0] == 0:
            continue
        assert np.array_equal(res.lo[k], P.min(axis=0)) and np.array_equal(res.hi[k], P.max(axis=0))
        t = (P.astype(np.float64) - res.center[k].astype(np.float64)) @ res.axes[k].astype(np.float64).T
        assert (np.abs(t) <= res.extent[k].astype(np.float64) / 2 + tol).all(), (k, np.abs(t).max(axis=0), res.extent[k])
        assert (res.extent[k][0] >= res.extent[k][2] - tol) or P.shape[0] < 8


def test_permuting_the_ids_permutes_the_rows():
    from randlanet.utils.boxes import instance_boxes_host
    xyz, ids, _ = bi.case("chunk_edges")
    want = bi.twin("chunk_edges")
    perm = np.array([3, 0, 4, 1, 2])                 # id k becomes perm[k]
    got = instance_boxes_host(xyz, np.where(ids >= 0, perm[np.maximum(ids, 0)], ids))
    for a, b in zip(got, want):
        assert np.array_equal(a[perm], b)
    # and the points of the other ids, and their order among them, do not matter either
    keep = np.flatnonzero((ids == 3) | (ids == -1))
    alone = instance_boxes_host(xyz[keep], ids[keep], 5)
    for a, b in zip(alone, want):
        assert np.array_equal(a[3], b[3])


def test_fixed_sum_follows_the_written_order():
    """fixed_sums against a scalar restatement of the contract, at lengths around the lane, the chunk and 64 chunks."""
    from randlanet.utils import boxes as B

    def by_hand(v):
        def fold(s):
            h = 32
            while h:
                s = [s[l] + s[l + h] for l in range(h)]
                h //= 2
            return s[0]

        def level(terms):
            lanes = [0.0] * 64
            for w, x in enumerate(terms):
                lanes[w % 64] = lanes[w % 64] + x
            return fold(lanes)
        return level([level(v[c:c + B.CHUNK]) for c in range(0, len(v), B.CHUNK)])

    rs = np.random.RandomState(0)
    sizes = [1, 63, 64, 65, B.CHUNK - 1, B.CHUNK, B.CHUNK + 1, 0, 3 * B.CHUNK + 5, 65 * B.CHUNK + 7]
    v = (rs.randn(sum(sizes)) * 10.0 ** rs.randint(-3, 6, sum(sizes)))
    got = B.fixed_sums(v[:, None], np.array(sizes))
    first = 0
    for k, n in enumerate(sizes):
        want = by_hand(v[first:first + n].tolist()) if n else 0.0
        assert got[k, 0] == want, (n, got[k, 0], want)
        first += n
    assert B.CHUNK == 1024 and B.TURNS * B.LANES == B.CHUNK


# ------------------------------------------------------------------------------------------------ 3. degenerate ids
def test_one_member_and_identical_members():
    from randlanet.utils.boxes import instance_boxes_host
    res = bi.twin("single_point")
    p = bi.case("single_point")[0][0]
    for r, n in ((res, 1), (instance_boxes_host(np.tile(p, (3000, 1)), np.zeros(3000, np.int64)), 3000)):
        assert r.count.tolist() == [n]
        assert np.array_equal(r.center[0], p) and np.array_equal(r.lo[0], p) and np.array_equal(r.hi[0], p)
        assert np.array_equal(r.axes[0], np.eye(3, dtype=F32))
        assert np.array_equal(r.extent[0], np.zeros(3, F32)) and np.array_equal(r.eigenvalues[0], np.zeros(3, F32))
    dup = bi.twin("duplicates")
    assert np.array_equal(dup.axes[2], np.eye(3, dtype=F32)) and not dup.extent[2].any()
    assert np.array_equal(dup.center[2], np.array([7.0, -3.5, 0.125], F32))
    assert (dup.extent[:2] > 1).all()


def test_two_members_collinear_and_coplanar():
    res = bi.twin("flat_and_thin")
    tol = 1e-5
    # id 4: two members (0, 0, 0) and (3, 4, 12): rank 1, the axis is the line, the extent its length 13
    assert res.count[4] == 2
    assert np.abs(res.axes[4, 0] - np.array([3, 4, 12]) / 13).max() < 1e-6
    assert abs(res.extent[4, 0] - 13) < tol and (np.abs(res.extent[4, 1:]) < tol).all()
    assert np.abs(res.center[4] - np.array([1.5, 2, 6])).max() < tol
    assert res.eigenvalues[4, 0] == pytest.approx(169 / 4, rel=1e-6) and (np.abs(res.eigenvalues[4, 1:]) < 1e-9).all()
    # ids 2, 3: collinear - along y exactly, and along (1, 2, -0.5)
    assert np.array_equal(res.axes[2, 0], np.array([0, 1, 0], F32)) and not res.extent[2, 1:].any()
    assert np.array_equal(res.center[2][[0, 2]], np.array([-1, 4], F32))
    d = np.array([1, 2, -0.5]) / np.linalg.norm([1, 2, -0.5])
    assert np.abs(res.axes[3, 0] - d).max() < 1e-6 and (np.abs(res.extent[3, 1:]) < tol).all() and res.extent[3, 0] > 20
    # ids 0, 1: coplanar - z = 2.5 exactly, and a tilted plane: two long axes, a third extent of rounding only
    assert np.array_equal(np.abs(res.axes[0, 2]), np.array([0, 0, 1], F32)) and res.extent[0, 2] == 0
    assert res.center[0, 2] == F32(2.5) and (res.extent[0, :2] > 15).all()
    assert (res.extent[1, :2] > 15).all() and 0 <= res.extent[1, 2] < tol
    assert res.eigenvalues[1, 2] < 1e-10 < res.eigenvalues[1, 1]


def test_an_id_without_members_and_no_id_at_all():
    res = bi.twin("gaps")
    assert res.count.shape == (14,) and res.count.tolist() == [0, 700, 0, 0, 1300, 0, 0, 0, 0, 2100, 0, 0, 0, 0]
    for k in np.flatnonzero(res.count == 0):
        assert (res.lo[k] == np.inf).all() and (res.hi[k] == -np.inf).all()
        assert not res.extent[k].any() and not res.center[k].any() and not res.eigenvalues[k].any()
        assert np.array_equal(res.axes[k], np.eye(3, dtype=F32))
    none = bi.twin("all_minus_one")
    assert none.count.tolist() == [0, 0, 0] and (none.lo == np.inf).all()
    from randlanet.utils.boxes import instance_boxes_host
    empty = instance_boxes_host(np.zeros((5, 3)), np.full(5, -7))        # max(ids) + 1 <= 0: no box
    assert empty.count.shape == (0,) and empty.axes.shape == (0, 3, 3) and empty.axes.dtype == F32


# ---------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals():
    from randlanet.utils.boxes import instance_boxes, instance_boxes_host
    xyz, ids = np.zeros((10, 3), F32), np.arange(10) % 3

    class Huge:                                      # a shape is all the check may look at
        shape = (2 ** 31 - 1, 3)

    for fn in (instance_boxes_host, lambda *a: instance_boxes(*a, device="cpu")):
        for bad_xyz in (np.zeros((10, 2)), np.zeros(10), np.zeros((0, 3)), np.zeros((2, 10, 3))):
            with pytest.raises(ValueError, match="xyz has shape|M=0 points"):
                fn(bad_xyz, ids[:bad_xyz.shape[0]])
        with pytest.raises(ValueError, match=r"outside 1 \.\. 2\^31 - 2"):
            fn(Huge(), ids)
        for bad_ids in (ids[:9], ids.astype(np.float64), ids.reshape(10, 1), ids.astype(bool)):
            with pytest.raises(ValueError, match="ids have shape"):
                fn(xyz, bad_ids)
        for v in (np.nan, np.inf, -np.inf, 1e39):
            bad = xyz.astype(np.float64)
            bad[4, 1] = v
            with pytest.raises(ValueError, match="non-finite coordinates, first at point 4"):
                fn(bad, ids)
        for n in (0, -1, 2, 2.5, True):
            with pytest.raises(ValueError, match="n_ids"):
                fn(xyz, ids, n)
        with pytest.raises(ValueError, match="ids, outside"):
            fn(xyz, ids, 2 ** 31 - 1)
        assert fn(xyz, ids, 3).count.tolist() == [4, 3, 3] and fn(xyz, ids.astype(np.uint8), 5).count.shape == (5,)


def test_new_entries_are_exported_and_check_their_arguments_on_the_host():
    from randlanet import _hip
    for n in ("rl_boxes_workspace_bytes", "rl_boxes_sort", "rl_boxes_moments", "rl_boxes_fit"):
        assert n in _hip.EXPORTS
    bi.abi_refusals(_hip.lib(), 1 << 20)             # never dereferenced: every call is refused before a launch


# -------------------------------------------------------------------------------------------------- 5. box metrics
def _cube(x, side=1.0):
    lo = np.array([x, 0.0, 0.0])
    return lo, lo + side


def _scene(cubes):
    lo = np.array([c[0] for c in cubes]).reshape(-1, 3)
    hi = np.array([c[1] for c in cubes]).reshape(-1, 3)
    return lo, hi


def test_box_iou_aligned():
    from randlanet.utils.box_metrics import box_iou_aligned
    lo_a, hi_a = _scene([_cube(0), _cube(10), (np.full(3, np.inf), np.full(3, -np.inf))])
    lo_b, hi_b = _scene([_cube(0.5), _cube(0), _cube(1.0), _cube(0, 2.0)])
    iou = box_iou_aligned(lo_a, hi_a, lo_b, hi_b)
    assert iou.shape == (3, 4) and iou.dtype == np.float64
    assert iou[0].tolist() == [0.5 / 1.5, 1.0, 0.0, 1.0 / 8.0]
    assert not iou[1].any() and not iou[2].any()                         # disjoint; empty
    assert box_iou_aligned(lo_a[:0], hi_a[:0], lo_b, hi_b).shape == (0, 4)
    flat = np.array([[0.0, 0, 0]]), np.array([[1.0, 1, 0]])              # no volume: the union is 0
    assert box_iou_aligned(*flat, *flat).tolist() == [[0.0]]
    with pytest.raises(ValueError):
        box_iou_aligned(lo_a, hi_a[:2], lo_b, hi_b)


def test_box_ap_known_by_construction():
    from randlanet.utils.box_metrics import BoxEvaluator
    gt = _scene([_cube(0), _cube(5), _cube(10)])
    cls = np.array([1, 1, 1])

    def ap(pred, scores, classes=None, **kw):
        ev = BoxEvaluator(3, **kw)
        lo, hi = _scene(pred)
        ev.add(lo, hi, np.ones(len(pred), np.int64) if classes is None else classes, np.asarray(scores, np.float64), *gt, cls)
        return ev.result()

    r = ap([_cube(0), _cube(5), _cube(10)], [0.9, 0.8, 0.7])             # perfect match
    assert r["box_AP25"] == r["box_AP50"] == r["class 1 box_AP50"] == 1.0
    assert np.isnan(r["class 0 box_AP50"]) and np.isnan(r["class 2 box_AP25"])      # ignored; no ground truth
    assert r["class 1 box_n_gt"] == 3 and r["class 1 box_n_pred"] == 3 and r["class 0 box_n_gt"] == 0
    r = ap([_cube(0), _cube(5)], [0.9, 0.8])                             # one miss: recall stops at 2 / 3
    assert r["box_AP50"] == pytest.approx(2 / 3) and r["box_AP25"] == pytest.approx(2 / 3)
    # one duplicate of the first box, scored between the others: TP, FP, TP, TP -> 1/3 * (1 + 3/4 + 3/4)
    r = ap([_cube(0), _cube(0), _cube(5), _cube(10)], [0.9, 0.85, 0.8, 0.7])
    assert r["box_AP50"] == pytest.approx((1 + 0.75 + 0.75) / 3)
    # the score order matters: a false positive first lowers the whole curve, last it costs nothing
    miss = _cube(20)
    # (precision 1/2, 2/3, 3/4 at recall 1/3, 2/3, 1: the envelope is 3/4 throughout)
    assert ap([miss, _cube(0), _cube(5), _cube(10)], [0.95, 0.9, 0.8, 0.7])["box_AP50"] == pytest.approx(3 / 4)
    assert ap([miss, _cube(0), _cube(5), _cube(10)], [0.1, 0.9, 0.8, 0.7])["box_AP50"] == 1.0
    # IoU 1/3 (shifted by half a side): a match at 0.25, none at 0.5; the threshold itself counts as a match
    r = ap([_cube(0.5), _cube(5), _cube(10)], [0.9, 0.8, 0.7])
    assert r["box_AP25"] == 1.0 and r["box_AP50"] == pytest.approx((0 + 2 / 3 + 2 / 3) / 3 + 0)
    # the better of two overlapping boxes is taken first by the higher score, the other one keeps what is left
    shifted = (np.array([0.0, 0, 0]), np.array([1.0, 1, 0.5]))           # IoU 0.5 exactly with the first box
    assert ap([shifted, _cube(5), _cube(10)], [0.9, 0.8, 0.7])["box_AP50"] == 1.0
    # a prediction of another class matches nothing; one of an ignored class is not scored at all
    r = ap([_cube(0), _cube(5), _cube(10)], [0.9, 0.8, 0.7], classes=np.array([1, 2, 0]))
    assert r["class 1 box_AP50"] == pytest.approx(1 / 3) and r["class 2 box_n_pred"] == 1 and np.isnan(r["class 2 box_AP50"])
    assert r["class 0 box_n_pred"] == 0 and r["box_AP50"] == pytest.approx(1 / 3)
    with pytest.raises(ValueError, match="class names"):
        BoxEvaluator(3).result(["a"])


def test_box_ap_ignored_class_min_gt_points_and_empty_sides():
    from randlanet.utils.box_metrics import BoxEvaluator
    lo, hi = _scene([_cube(0), _cube(5), _cube(10)])
    none = np.zeros((0, 3))
    # class 2 ignored: its ground truth and its predictions do not exist
    ev = BoxEvaluator(3, ignore_classes=(0, 2))
    ev.add(lo, hi, np.array([1, 2, 2]), np.array([0.9, 0.8, 0.7]), lo, hi, np.array([1, 2, 1]))
    r = ev.result(["void", "chair", "table"])
    assert r["chair box_AP50"] == pytest.approx(1 / 2) and np.isnan(r["table box_AP50"]) and r["table box_n_gt"] == 0
    assert r["box_AP50"] == pytest.approx(1 / 2) and list(r)[:2] == ["box_AP25", "box_AP50"]
    # min_gt_points: the small box is no positive, and the prediction on it is neither TP nor FP
    ev = BoxEvaluator(2, min_gt_points=10)
    ev.add(lo, hi, np.ones(3, np.int64), np.array([0.9, 0.8, 0.7]), lo, hi, np.ones(3, np.int64), np.array([100, 9, 10]))
    r = ev.result()
    assert r["class 1 box_n_gt"] == 2 and r["box_AP50"] == 1.0
    ev = BoxEvaluator(2, min_gt_points=10)
    ev.add(lo[1:2], hi[1:2], np.ones(1, np.int64), np.array([0.9]), lo, hi, np.ones(3, np.int64), np.array([100, 9, 10]))
    assert ev.result()["box_AP50"] == 0.0            # only the ignored box was found: no TP, no FP, two misses
    # no prediction: 0 with ground truth; no ground truth: NaN; empty boxes on either side do not exist
    ev = BoxEvaluator(2)
    ev.add(none, none, np.zeros(0, np.int64), np.zeros(0), lo, hi, np.ones(3, np.int64))
    assert ev.result()["box_AP25"] == 0.0
    ev = BoxEvaluator(2)
    ev.add(lo, hi, np.ones(3, np.int64), np.array([0.9, 0.8, 0.7]), none, none, np.zeros(0, np.int64))
    assert np.isnan(ev.result()["box_AP25"]) and ev.result()["class 1 box_n_pred"] == 3
    ev = BoxEvaluator(2)
    inf = np.full((1, 3), np.inf)
    ev.add(np.concatenate((lo, inf)), np.concatenate((hi, -inf)), np.ones(4, np.int64), np.array([0.9, 0.8, 0.7, 0.99]),
           np.concatenate((inf, lo)), np.concatenate((-inf, hi)), np.ones(4, np.int64))
    r = ev.result()
    assert r["box_AP50"] == 1.0 and r["class 1 box_n_gt"] == 3 and r["class 1 box_n_pred"] == 3
    # scenes are matched apart and ranked together
    ev = BoxEvaluator(2)
    ev.add(lo[:1], hi[:1], np.ones(1, np.int64), np.array([0.5]), lo[:1], hi[:1], np.ones(1, np.int64))
    ev.add(lo[:1], hi[:1], np.ones(1, np.int64), np.array([0.9]), lo[1:2], hi[1:2], np.ones(1, np.int64))
    assert ev.result()["box_AP50"] == pytest.approx(1 / 2 * 1 / 2)       # FP (0.9) first, then the TP: precision 1/2


# ------------------------------------------------------------------------------------------------ 6. CPU-placed model
@pytest.fixture(scope="module")
def cpu_model():
    from randlanet.model import Model
    from randlanet.utils.modules import RandLANetSettings
    torch.manual_seed(0)
    return Model(RandLANetSettings(n_classes=4, n_points=1024, n_neighbors=8, layer_sizes=[8, 16, 32, 32]), use_gpu=False)


@pytest.mark.parametrize("grid", [None, 0.3])
def test_predict_instances_with_oriented_boxes_on_a_cpu_model(cpu_model, grid):
    from randlanet.utils.boxes import instance_boxes_host
    xyz = np.random.RandomState(7).uniform(0, 6, (3000, 3)).astype(F32)
    kw = dict(radius=0.45, min_points=2, ignore_classes=(3,), min_confidence=0.26, votes=1, batch_size=2, seed=2, grid=grid)
    np.random.seed(5)
    plain = cpu_model.predict_instances(xyz, **kw)
    np.random.seed(5)
    off = cpu_model.predict_instances(xyz, oriented_boxes=False, **kw)
    np.random.seed(5)
    got = cpu_model.predict_instances(xyz, oriented_boxes=True, **kw)
    assert type(plain).__name__ == type(off).__name__ == "InstanceResult" and len(plain) == 8
    assert type(got).__name__ == "OrientedInstanceResult"
    assert got._fields == plain._fields + ("box_center", "box_axes", "box_extent", "box_eigenvalues")
    for a, b, c in zip(plain, off, got[:8]):
        assert np.array_equal(a, b) and np.array_equal(a, c) and a.dtype == c.dtype
    I = plain.count.shape[0]
    assert I >= 2
    want = instance_boxes_host(xyz, plain.instance, I)
    for a, b in zip(got[8:], (want.center, want.axes, want.extent, want.eigenvalues)):
        assert np.array_equal(a, b) and a.dtype == F32
    if grid is None:                                 # over the raw points: the clustering's own count and box
        assert np.array_equal(want.count, plain.count)
        assert np.array_equal(want.lo, plain.lo) and np.array_equal(want.hi, plain.hi)
    else:
        assert (want.count >= plain.count).all() and want.count.sum() == (plain.instance >= 0).sum()


def test_evaluate_instances_with_boxes_on_a_cpu_model(cpu_model):
    from randlanet.utils.box_metrics import BoxEvaluator
    from randlanet.utils.boxes import instance_boxes_host
    rs = np.random.RandomState(11)
    scenes = []
    for M in (3000, 2500):
        xyz = rs.uniform(0, 5, (M, 3)).astype(F32)
        ids = (np.floor(xyz[:, 0] / 2.5) + 2 * np.floor(xyz[:, 1] / 2.5)).astype(np.int64) * 5
        labels = ids // 5 % 4
        ids[xyz[:, 2] > 4.8] = -1
        scenes.append((xyz, None, labels, ids))
    kw = dict(radius=0.45, min_points=2, ignore_classes=(3,), min_confidence=0.26, votes=1, batch_size=2, seed=2)
    np.random.seed(5)
    plain = cpu_model.evaluate_instances(scenes, **kw)
    np.random.seed(5)
    off = cpu_model.evaluate_instances(scenes, boxes=False, **kw)
    np.random.seed(5)
    got = cpu_model.evaluate_instances(scenes, boxes=True, **kw)
    assert list(plain) == list(off) and not any(k.startswith("box_") or " box_" in k for k in plain)
    assert list(got)[:len(plain)] == list(plain)
    for k in plain:
        assert got[k] == plain[k] == off[k] or (np.isnan(got[k]) and np.isnan(plain[k]) and np.isnan(off[k]))
    # the box scores by hand: predictions and ground truth through instance_boxes_host, classes by majority
    np.random.seed(5)
    ev = BoxEvaluator(4, ignore_classes=(3,))
    for xyz, _, labels, ids in scenes:
        res = cpu_model.predict_instances(xyz, **kw)
        pred = instance_boxes_host(xyz, res.instance, max(res.count.shape[0], 1))
        g = np.where(labels == 3, -1, ids)
        gt = instance_boxes_host(xyz, g, int(g.max()) + 1)
        gt_class = np.array([np.bincount(labels[g == k]).argmax() if (g == k).any() else -1 for k in range(gt.count.shape[0])])
        ev.add(pred.lo[:res.count.shape[0]], pred.hi[:res.count.shape[0]], res.classes, res.score, gt.lo, gt.hi, gt_class)
    want = ev.result()
    assert [k for k in got if k not in plain] == list(want)
    for k, v in want.items():
        assert got[k] == v or (np.isnan(got[k]) and np.isnan(v)), k
    assert got["class 0 box_n_gt"] + got["class 1 box_n_gt"] + got["class 2 box_n_gt"] == 6 and np.isnan(got["class 3 box_AP25"])
