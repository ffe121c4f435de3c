"""Scoring predicted instances against ground-truth instances: the step after Model.predict_instances that says whether a
setting of radius, min_points, min_confidence and ignore_classes is good - average precision at IoU thresholds (the ScanNet
protocol's AP, AP50, AP25), precision and recall at 0.5, and the coverage scores mCov / mWCov of the S3DIS instance papers.

The only part that scales with the number of points is the sparse contingency table of two integer id arrays:

  pair_counts   a, b (M,) integers, 1 <= M < 2^31 - 1, ids below A (below B), 1 <= A, B <= 2^31 - 1.  A value below -1 counts
                as -1; a value >= A (>= B) is a ValueError, and so is (A + 1) * (B + 1) > 2^62.  Result (pa, pb int32, count
                int64): every pair (a_i, b_i) that occurs, once, in ascending order of (a, b) with -1 first, and how many points
                carry it; count.sum() == M.  pair_counts_host is the numpy twin and the specification of csrc/pairs.hip
                (include/rl_randlanet.h, rl_pairs_*); the kernels are integer work only and equal it exactly

Everything downstream of the tables is small and runs on the host in float64, the same code for both paths, so the device path
and the host path differ in an integer table only.  Per scene (InstanceEvaluator.add):

  ground truth  g'_i = gt_instance_i where gt_instance_i >= 0 and gt_labels_i is inside [0, n_classes) and not ignored, else
                -1; G = max(gt_instance) + 1.  Ids need not be dense: an id without points does not exist.  The class of a
                ground-truth instance is its most frequent label, ties to the lowest (pair_counts(g', label', G, n_classes))
  overlaps      pair_counts(pred_instance, g', I, G) over the raw points; |p| = the sum of p's row (the -1 column included),
                |g| = the sum of g's column (the -1 row included), IoU(p, g) = n_pg / (|p| + |g| - n_pg), one division
  ignored       a ground-truth instance with |g| < min_gt_points is no positive, and a prediction matched to it is dropped
  void          void_p = the points of p with g' = -1 or lying in an ignored ground-truth instance
  matching      at threshold t, per class: the predictions in descending score (ties: ascending number) each take the not
                yet taken, non-ignored ground-truth instance of their class with the largest IoU among those with IoU > t
                (strictly; ties to the lowest id) - a TP.  Otherwise the prediction is dropped when it has IoU > t with an
                ignored instance of its class or void_p / |p| > t, and is an FP if not

result() pools the scenes: per class and threshold the kept predictions in descending score (ties: scene order, then number),
precision and recall over N_pos (the non-ignored ground-truth instances of the class), AP = the area under the precision
envelope (all points).  AP is NaN without ground truth and 0 with ground truth and no prediction; means skip NaN.
"""
from collections import OrderedDict

import numpy as np

from . import grid as G

MAX_IDS = (1 << 31) - 1         # pa, pb are int32
MAX_KEY = 1 << 62
DEFAULT_THRESHOLDS = tuple(round(0.5 + 0.05 * k, 2) for k in range(10))


# ------------------------------------------------------------------------------------------------------ pair counts
def check_pairs(a, b, A, B):
    """The refusals of pair_counts that need no pass over the values, all ValueError.  Returns (a, b) as numpy arrays of their
    own integer dtype and A, B as int."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 1 or a.dtype.kind not in "iu":
        raise ValueError(f"pair_counts: a has shape {tuple(a.shape)} and dtype {a.dtype}, expected (M,) integers")
    M = a.shape[0]
    if b.shape != (M,) or b.dtype.kind not in "iu":
        raise ValueError(f"pair_counts: b has shape {tuple(b.shape)} and dtype {b.dtype}, expected ({M},) integers")
    if M == 0 or M >= G.MAX_POINTS:
        raise ValueError(f"pair_counts: M={M} points, outside 1 .. 2^31 - 2")
    A, B = check_bounds(A, B)
    return a, b, A, B


def check_bounds(A, B):
    if int(A) != A or int(B) != B or int(A) < 1 or int(B) < 1:
        raise ValueError(f"pair_counts: A={A!r}, B={B!r} must be integers >= 1")
    A, B = int(A), int(B)
    if (A + 1) * (B + 1) > MAX_KEY:
        raise ValueError(f"pair_counts: (A + 1) * (B + 1) = {(A + 1) * (B + 1)} exceeds 2^62")
    if A > MAX_IDS or B > MAX_IDS:
        raise ValueError(f"pair_counts: A={A}, B={B} exceed 2^31 - 1, the ids of the result are int32")
    return A, B


def out_of_range(A: int, B: int) -> ValueError:
    return ValueError(f"pair_counts: a value is out of range (a >= A={A} or b >= B={B})")


def key_bits(A: int, B: int) -> int:
    """Bits of the largest key (A + 1) * (B + 1) - 1, at least 1: the sort runs ceil(bits / 8) digit passes."""
    return max(1, ((A + 1) * (B + 1) - 1).bit_length())


def pair_counts_host(a, b, A, B):
    """The numpy twin of the device pair counts; see the module docstring for the contract."""
    a, b, A, B = check_pairs(a, b, A, B)
    if int(a.max()) >= A or int(b.max()) >= B:
        raise out_of_range(A, B)
    a = np.maximum(a.astype(np.int64), -1)
    b = np.maximum(b.astype(np.int64), -1)
    key = (a + 1) * (B + 1) + (b + 1)
    u, n = np.unique(key, return_counts=True)
    return (u // (B + 1) - 1).astype(np.int32), (u % (B + 1) - 1).astype(np.int32), n.astype(np.int64)


def _device_ids(x: np.ndarray):
    """int32 stays int32 (half the upload), every other integer type goes up as int64."""
    return np.require(x, requirements="CW") if x.dtype == np.int32 else x.astype(np.int64)


def pair_counts(a, b, A, B, device=None):
    """(pa (P,) int32, pb (P,) int32, count (P,) int64): the pairs (a_i, b_i) that occur among the (M,) integer arrays a and
    b, in ascending order of (a, b) with -1 first, and their number of points.  Runs on the GPU (csrc/pairs.hip) when
    `device` is a cuda device, or when it is None and one is available; otherwise pair_counts_host.  Either way the result
    is numpy arrays, and the same ones."""
    import torch
    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device(device)
    if device.type != "cuda":
        return pair_counts_host(a, b, A, B)
    from .. import _ops as ops
    a, b, A, B = check_pairs(a, b, A, B)
    if a.dtype.kind == "u" and int(a.max()) >= A or b.dtype.kind == "u" and int(b.max()) >= B:
        raise out_of_range(A, B)                        # (before an unsigned value can wrap in the conversion)
    with torch.cuda.device(device), torch.no_grad():
        res = ops.pair_counts(torch.from_numpy(_device_ids(a)).to(device), torch.from_numpy(_device_ids(b)).to(device), A, B)
        return tuple(t.cpu().numpy() for t in res)


# ---------------------------------------------------------------------------------------------------------- scoring
def average_precision(tp: np.ndarray, n_pos: int) -> float:
    """The area under the precision envelope (all-point interpolation) of predictions already in descending score; tp (n,)
    bool.  NaN without positives, 0 without predictions."""
    if n_pos == 0:
        return float("nan")
    if tp.shape[0] == 0:
        return 0.0
    ctp = np.cumsum(tp).astype(np.float64)
    cfp = np.cumsum(~tp).astype(np.float64)
    rec = np.concatenate(([0.0], ctp / float(n_pos), [1.0]))
    pre = np.concatenate(([0.0], ctp / (ctp + cfp), [0.0]))
    pre = np.maximum.accumulate(pre[::-1])[::-1]
    step = np.flatnonzero(rec[1:] != rec[:-1])
    return float(np.sum((rec[step + 1] - rec[step]) * pre[step + 1]))


def _mean(values) -> float:
    v = [x for x in values if not np.isnan(x)]
    return float(np.mean(v)) if v else float("nan")


class InstanceEvaluator:
    """Accumulates scenes (add) and scores them (result); see the module docstring for the protocol.  `device`: where the
    pair counts run - a cuda device (or None with one available) runs csrc/pairs.hip, anything else the numpy twin; the
    scores are the same floats either way."""

    def __init__(self, n_classes: int, *, ignore_classes=(0,), min_gt_points: int = 1, iou_thresholds=None, device=None):
        import torch
        if int(n_classes) != n_classes or int(n_classes) < 1:
            raise ValueError(f"InstanceEvaluator: n_classes={n_classes!r} must be an integer >= 1")
        if int(min_gt_points) != min_gt_points or int(min_gt_points) < 1:
            raise ValueError(f"InstanceEvaluator: min_gt_points={min_gt_points!r} must be an integer >= 1")
        self.n_classes, self.min_gt_points = int(n_classes), int(min_gt_points)
        ignore = np.asarray(tuple(ignore_classes) if ignore_classes is not None else (), dtype=np.int64)
        if ignore.ndim != 1:
            raise ValueError(f"InstanceEvaluator: ignore_classes has shape {tuple(ignore.shape)}, expected a flat sequence")
        self.ignore = np.unique(ignore)
        self.classes = [c for c in range(self.n_classes) if c not in set(self.ignore.tolist())]
        ap = DEFAULT_THRESHOLDS if iou_thresholds is None else tuple(float(t) for t in iou_thresholds)
        if not ap or any(not 0.0 <= t < 1.0 for t in ap):
            raise ValueError(f"InstanceEvaluator: iou_thresholds={iou_thresholds!r} must be a sequence inside [0, 1)")
        self.ap_thresholds = ap                                  # "AP" is the mean over these
        self.thresholds = tuple(sorted(set(ap) | {0.25, 0.5}))   # AP25 and AP50 are always reported
        if device is None:
            device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.scenes = 0
        # per class: N_pos, predictions seen, coverage sums; per (class, threshold): (score, scene, number, tp) of the kept
        self.n_pos = {c: 0 for c in self.classes}
        self.n_pred = {c: 0 for c in self.classes}
        self.cov = {c: [0.0, 0.0, 0.0] for c in self.classes}    # sum of best IoU, sum of |g| * best IoU, sum of |g|
        self.kept = {(c, t): [] for c in self.classes for t in self.thresholds}

    # ------------------------------------------------------------------------------------------------- the tables
    def _pairs(self, a, b, A: int, B: int):
        import torch
        if self.device.type != "cuda":
            a = a.cpu().numpy() if torch.is_tensor(a) else a
            return pair_counts_host(a, b, A, B)
        from .. import _ops as ops
        check_bounds(A, B)
        with torch.cuda.device(self.device), torch.no_grad():
            ta = a.to(self.device) if torch.is_tensor(a) else torch.from_numpy(_device_ids(a)).to(self.device)
            tb = torch.from_numpy(_device_ids(b)).to(self.device)
            return tuple(t.cpu().numpy() for t in ops.pair_counts(ta.contiguous(), tb, A, B))

    def add(self, pred_instance, pred_classes, pred_scores, gt_instance, gt_labels) -> None:
        """One scene: pred_instance (M,) integers - the predicted instance of every point, -1 for none; a numpy array or a
        tensor on this evaluator's device -, pred_classes (I,) integers and pred_scores (I,) per predicted instance,
        gt_instance (M,) and gt_labels (M,) integers.  Refusals are ValueError."""
        import torch
        gi, gl = np.asarray(gt_instance), np.asarray(gt_labels)
        if gi.ndim != 1 or gi.dtype.kind not in "iu":
            raise ValueError(f"InstanceEvaluator.add: gt_instance has shape {tuple(gi.shape)} and dtype {gi.dtype}, "
                             "expected (M,) integers")
        M = gi.shape[0]
        if M == 0 or M >= G.MAX_POINTS:
            raise ValueError(f"InstanceEvaluator.add: M={M} points, outside 1 .. 2^31 - 2")
        if gl.shape != (M,) or gl.dtype.kind not in "iu":
            raise ValueError(f"InstanceEvaluator.add: gt_labels have shape {tuple(gl.shape)} and dtype {gl.dtype}, "
                             f"expected ({M},) integers")
        if torch.is_tensor(pred_instance):
            pi = pred_instance
            if tuple(pi.shape) != (M,) or pi.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"InstanceEvaluator.add: pred_instance has shape {tuple(pi.shape)} and dtype {pi.dtype}, "
                                 f"expected ({M},) int32 or int64")
        else:
            pi = np.asarray(pred_instance)
            if pi.shape != (M,) or pi.dtype.kind not in "iu":
                raise ValueError(f"InstanceEvaluator.add: pred_instance has shape {tuple(pi.shape)} and dtype {pi.dtype}, "
                                 f"expected ({M},) integers")
        pc = np.asarray(pred_classes)
        if pc.ndim != 1 or (pc.size and pc.dtype.kind not in "iu"):
            raise ValueError(f"InstanceEvaluator.add: pred_classes have shape {tuple(pc.shape)} and dtype {pc.dtype}, "
                             "expected (I,) integers")
        I = pc.shape[0]
        ps = np.asarray(pred_scores, dtype=np.float64)
        if ps.shape != (I,):
            raise ValueError(f"InstanceEvaluator.add: pred_scores have shape {tuple(ps.shape)}, expected ({I},)")
        pc = pc.astype(np.int64)
        C = self.n_classes

        gi, gl = gi.astype(np.int64), gl.astype(np.int64)
        valid = (gi >= 0) & (gl >= 0) & (gl < C) & ~np.isin(gl, self.ignore)
        g1, l1 = np.where(valid, gi, -1), np.where(valid, gl, -1)
        n_gt = max(int(gi.max()) + 1, 1)

        # the class of every ground-truth instance: the most frequent label, ties to the lowest (the rows come in ascending
        # (g, label), so "strictly more" keeps the lowest)
        ga, la, n = self._pairs(g1, l1, n_gt, C)
        gt_class = np.full(n_gt, -1, np.int64)
        most = np.zeros(n_gt, np.int64)
        for g, l, k in zip(ga.tolist(), la.tolist(), n.tolist()):
            if g >= 0 and l >= 0 and k > most[g]:
                most[g], gt_class[g] = k, l

        pa, pb, n = self._pairs(pi, g1, max(I, 1), n_gt)
        pa, pb = pa.astype(np.int64), pb.astype(np.int64)
        if I == 0 and (pa >= 0).any():
            raise ValueError("InstanceEvaluator.add: pred_instance names an instance, pred_classes is empty")
        size_p, size_g = np.zeros(max(I, 1), np.int64), np.zeros(n_gt, np.int64)
        np.add.at(size_p, pa[pa >= 0], n[pa >= 0])
        np.add.at(size_g, pb[pb >= 0], n[pb >= 0])
        ignored = (size_g > 0) & (size_g < self.min_gt_points)
        void = np.zeros(max(I, 1), np.int64)
        in_void = (pa >= 0) & ((pb < 0) | ignored[np.maximum(pb, 0)])
        np.add.at(void, pa[in_void], n[in_void])
        both = (pa >= 0) & (pb >= 0)
        op, og, on = pa[both], pb[both], n[both]                     # ascending (p, g)
        iou = on.astype(np.float64) / (size_p[op] + size_g[og] - on).astype(np.float64)
        first = np.searchsorted(op, np.arange(max(I, 1) + 1))       # p's overlaps are first[p] .. first[p + 1]
        with np.errstate(invalid="ignore", divide="ignore"):
            void_share = np.where(size_p > 0, void / np.maximum(size_p, 1).astype(np.float64), 0.0)

        scene = self.scenes
        self.scenes += 1
        for c in self.classes:
            positives = np.flatnonzero((size_g > 0) & ~ignored & (gt_class == c))
            self.n_pos[c] += positives.size
            preds = [p for p in range(I) if pc[p] == c]
            self.n_pred[c] += len(preds)
            # coverage: the best IoU of every positive with a prediction of its class
            best = np.zeros(n_gt, np.float64)
            mine = (pc[op] == c) if op.size else np.zeros(0, bool)
            np.maximum.at(best, og[mine], iou[mine])
            for g in positives.tolist():
                self.cov[c][0] += best[g]
                self.cov[c][1] += float(size_g[g]) * best[g]
                self.cov[c][2] += float(size_g[g])
            preds.sort(key=lambda p: (-ps[p], p))
            cands = {p: [(int(og[j]), float(iou[j]), bool(ignored[og[j]])) for j in range(first[p], first[p + 1])
                         if gt_class[og[j]] == c] for p in preds}
            for t in self.thresholds:
                taken = set()
                rows = self.kept[(c, t)]
                for p in preds:
                    match, match_iou, near_ignored = -1, -1.0, False
                    for g, v, ign in cands[p]:
                        if not v > t:
                            continue
                        if ign:
                            near_ignored = True
                        elif g not in taken and v > match_iou:       # strictly: ties stay with the lowest id
                            match, match_iou = g, v
                    if match >= 0:
                        taken.add(match)
                        rows.append((ps[p], scene, p, True))
                    elif near_ignored or void_share[p] > t:
                        continue                                     # dropped: neither TP nor FP
                    else:
                        rows.append((ps[p], scene, p, False))

    # -------------------------------------------------------------------------------------------------- the scores
    def result(self, class_names=None) -> OrderedDict:
        """"AP" (the mean over the thresholds 0.50 .. 0.95, or over iou_thresholds), "AP50", "AP25", "precision50", "recall50",
        "mCov", "mWCov" - each the mean over the classes, NaN skipped - then per class "<class> AP", "... AP50", "... AP25",
        "... precision50", "... recall50", "... Cov", "... WCov", "... n_gt" and "... n_pred" ("class c" without names; an
        ignored class has NaN scores and zero counts)."""
        if class_names is not None and len(class_names) != self.n_classes:
            raise ValueError(f"InstanceEvaluator.result: {len(class_names)} class names for n_classes={self.n_classes}")
        nan = float("nan")
        per = {}
        for c in range(self.n_classes):
            if c not in self.n_pos:
                per[c] = dict(AP=nan, AP50=nan, AP25=nan, precision50=nan, recall50=nan, Cov=nan, WCov=nan, n_gt=0, n_pred=0)
                continue
            n_pos = self.n_pos[c]
            ap = {}
            for t in self.thresholds:
                rows = sorted(self.kept[(c, t)], key=lambda r: (-r[0], r[1], r[2]))
                tp = np.array([r[3] for r in rows], dtype=bool)
                ap[t] = average_precision(tp, n_pos)
                if t == 0.5:
                    n_tp = int(tp.sum())
                    precision = n_tp / tp.shape[0] if tp.shape[0] else nan
                    recall = n_tp / n_pos if n_pos else nan
            s, w, d = self.cov[c]
            per[c] = dict(AP=_mean([ap[t] for t in self.ap_thresholds]) if n_pos else nan, AP50=ap[0.5], AP25=ap[0.25],
                          precision50=precision, recall50=recall, Cov=s / n_pos if n_pos else nan,
                          WCov=w / d if n_pos else nan, n_gt=n_pos, n_pred=self.n_pred[c])
        out = OrderedDict()
        for key, col in (("AP", "AP"), ("AP50", "AP50"), ("AP25", "AP25"), ("precision50", "precision50"),
                         ("recall50", "recall50"), ("mCov", "Cov"), ("mWCov", "WCov")):
            out[key] = _mean([per[c][col] for c in range(self.n_classes)])
        for c in range(self.n_classes):
            name = class_names[c] if class_names else f"class {c}"
            for col, v in per[c].items():
                out[f"{name} {col}"] = v
        return out
