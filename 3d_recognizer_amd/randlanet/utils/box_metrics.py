"""Scoring predicted boxes against ground-truth boxes: the detection metric of the ScanNet and SUN RGB-D benchmarks, box
mAP@0.25 / mAP@0.5 over axis-aligned boxes - what Model.evaluate_instances(boxes=True) reports next to the mask metrics of
utils/instance_metrics.py.  Everything here is small - boxes, not points - and runs on the host in float64.

  box           lo, hi (3,): the corners.  A box with hi < lo on an axis is empty (the lo = +inf, hi = -inf of an id without
                points): it overlaps nothing, is no ground truth and no prediction
  IoU           per axis the overlap max(min(hi_a, hi_b) - max(lo_a, lo_b), 0); inter = their product, vol = the product of
                hi - lo, IoU = inter / (vol_a + vol_b - inter), one division; 0 where that denominator is not positive
  ground truth  of a scene: its non-empty boxes whose class is inside [0, n_classes) and not ignored.  One with fewer than
                min_gt_points points (gt_counts) is ignored: no positive, and a prediction matched to it is dropped
  matching      per class and threshold t, over ALL scenes: the predictions in descending score (ties: scene order, then
                number) each take the not yet taken ground-truth box of their scene and class with the largest IoU among those
                with IoU >= t (ties to the lowest number) - a TP when that box counts, dropped when it is ignored - and are an
                FP without one
  AP            instance_metrics.average_precision over the TP flags in that order and N_pos, the counted ground-truth boxes of
                the class: the area under the precision envelope.  NaN without ground truth, 0 with ground truth and no
                prediction; the means skip NaN
"""
from collections import OrderedDict

import numpy as np

from .instance_metrics import _mean, average_precision


def _boxes(lo, hi, what: str):
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    if lo.ndim != 2 or lo.shape[1] != 3 or hi.shape != lo.shape:
        raise ValueError(f"{what}: lo and hi have shapes {tuple(lo.shape)} and {tuple(hi.shape)}, expected (n, 3) both")
    if np.isnan(lo).any() or np.isnan(hi).any():
        raise ValueError(f"{what}: a corner is not a number")
    return lo, hi


def box_iou_aligned(lo_a, hi_a, lo_b, hi_b) -> np.ndarray:
    """(A, B) float64: the IoU of every axis-aligned box a = (lo_a, hi_a) (A, 3) with every b (B, 3); an empty box gives 0."""
    lo_a, hi_a = _boxes(lo_a, hi_a, "box_iou_aligned")
    lo_b, hi_b = _boxes(lo_b, hi_b, "box_iou_aligned")
    full_a, full_b = (hi_a >= lo_a).all(axis=1), (hi_b >= lo_b).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        side = np.minimum(hi_a[:, None, :], hi_b[None, :, :]) - np.maximum(lo_a[:, None, :], lo_b[None, :, :])
        inter = np.prod(np.maximum(side, 0.0), axis=2)
        vol_a, vol_b = np.prod(hi_a - lo_a, axis=1), np.prod(hi_b - lo_b, axis=1)
        union = vol_a[:, None] + vol_b[None, :] - inter
        ok = full_a[:, None] & full_b[None, :] & (union > 0.0) & np.isfinite(union)
        return np.where(ok, inter / np.where(ok, union, 1.0), 0.0)


class BoxEvaluator:
    """Accumulates scenes (add) and scores them (result); see the module docstring for the protocol."""

    def __init__(self, n_classes: int, ignore_classes=(0,), min_gt_points: int = 1, iou_thresholds=(0.25, 0.5)):
        if int(n_classes) != n_classes or int(n_classes) < 1:
            raise ValueError(f"BoxEvaluator: n_classes={n_classes!r} must be an integer >= 1")
        if int(min_gt_points) != min_gt_points or int(min_gt_points) < 1:
            raise ValueError(f"BoxEvaluator: min_gt_points={min_gt_points!r} must be an integer >= 1")
        self.n_classes, self.min_gt_points = int(n_classes), int(min_gt_points)
        ignore = np.asarray(tuple(ignore_classes) if ignore_classes is not None else (), dtype=np.int64)
        if ignore.ndim != 1:
            raise ValueError(f"BoxEvaluator: ignore_classes has shape {tuple(ignore.shape)}, expected a flat sequence")
        self.ignore = set(ignore.tolist())
        self.classes = [c for c in range(self.n_classes) if c not in self.ignore]
        th = tuple(float(t) for t in iou_thresholds)
        if not th or any(not 0.0 < t <= 1.0 for t in th):
            raise ValueError(f"BoxEvaluator: iou_thresholds={iou_thresholds!r} must be a sequence inside (0, 1]")
        self.thresholds = th
        self.scenes = 0
        self.n_pos = {c: 0 for c in self.classes}
        self.n_pred = {c: 0 for c in self.classes}
        # per class: (score, scene, number, row of IoUs with the scene's boxes of the class, their ignored flags, slot of them)
        self.preds = {c: [] for c in self.classes}
        self.n_gt = {c: [] for c in self.classes}                # per scene: the ground-truth boxes of the class

    def add(self, pred_lo, pred_hi, pred_classes, pred_scores, gt_lo, gt_hi, gt_classes, gt_counts=None) -> None:
        """One scene: pred_lo, pred_hi (P, 3), pred_classes (P,) integers, pred_scores (P,); gt_lo, gt_hi (G, 3), gt_classes
        (G,) integers and - for min_gt_points - gt_counts (G,), the points of every ground-truth box (None: every box counts).
        Empty boxes (hi < lo) are skipped on both sides.  Refusals are ValueError."""
        plo, phi = _boxes(pred_lo, pred_hi, "BoxEvaluator.add (predictions)")
        glo, ghi = _boxes(gt_lo, gt_hi, "BoxEvaluator.add (ground truth)")
        pc, gc = np.asarray(pred_classes), np.asarray(gt_classes)
        ps = np.asarray(pred_scores, dtype=np.float64)
        P, Gn = plo.shape[0], glo.shape[0]
        if pc.shape != (P,) or (P and pc.dtype.kind not in "iu") or ps.shape != (P,):
            raise ValueError(f"BoxEvaluator.add: pred_classes {tuple(pc.shape)} {pc.dtype} and pred_scores {tuple(ps.shape)}, "
                             f"expected ({P},) integers and ({P},)")
        if gc.shape != (Gn,) or (Gn and gc.dtype.kind not in "iu"):
            raise ValueError(f"BoxEvaluator.add: gt_classes have shape {tuple(gc.shape)} and dtype {gc.dtype}, expected "
                             f"({Gn},) integers")
        if gt_counts is None:
            small = np.zeros(Gn, bool)
        else:
            n = np.asarray(gt_counts)
            if n.shape != (Gn,):
                raise ValueError(f"BoxEvaluator.add: gt_counts have shape {tuple(n.shape)}, expected ({Gn},)")
            small = n < self.min_gt_points
        pc, gc = pc.astype(np.int64), gc.astype(np.int64)
        p_full, g_full = (phi >= plo).all(axis=1), (ghi >= glo).all(axis=1)
        iou = box_iou_aligned(plo, phi, glo, ghi)
        scene = self.scenes
        self.scenes += 1
        for c in self.classes:
            g = np.flatnonzero(g_full & (gc == c))
            self.n_pos[c] += int((~small[g]).sum())
            self.n_gt[c].append(g.size)
            for p in np.flatnonzero(p_full & (pc == c)).tolist():
                self.preds[c].append((ps[p], scene, p, iou[p, g], small[g]))
                self.n_pred[c] += 1

    def result(self, class_names=None) -> OrderedDict:
        """"box_AP25" and "box_AP50" (one "box_AP<100 t>" per threshold) - each the mean over the classes, NaN skipped -
        then per class "<class> box_AP25", "... box_AP50", "... box_n_gt" and "... box_n_pred" ("class c" without names; an
        ignored class has NaN scores and zero counts)."""
        if class_names is not None and len(class_names) != self.n_classes:
            raise ValueError(f"BoxEvaluator.result: {len(class_names)} class names for n_classes={self.n_classes}")
        keys = [f"box_AP{int(round(100 * t))}" for t in self.thresholds]
        per = {}
        for c in range(self.n_classes):
            if c not in self.n_pos:
                per[c] = {k: float("nan") for k in keys}
                per[c].update(box_n_gt=0, box_n_pred=0)
                continue
            rows = sorted(self.preds[c], key=lambda r: (-r[0], r[1], r[2]))
            per[c] = {}
            for key, t in zip(keys, self.thresholds):
                taken = [np.zeros(n, bool) for n in self.n_gt[c]]
                tp = []
                for _, scene, _, iou, small in rows:
                    v = np.where(taken[scene] | ~(iou >= t), -1.0, iou)
                    if v.size == 0 or v.max() < 0.0:
                        tp.append(False)
                        continue
                    g = int(np.argmax(v))                    # the first maximum: ties to the lowest number
                    taken[scene][g] = True
                    if not small[g]:
                        tp.append(True)                      # (a prediction on an ignored box is neither TP nor FP)
                per[c][key] = average_precision(np.asarray(tp, dtype=bool), self.n_pos[c])
            per[c].update(box_n_gt=self.n_pos[c], box_n_pred=self.n_pred[c])
        out = OrderedDict()
        for key in keys:
            out[key] = _mean([per[c][key] for c in range(self.n_classes)])
        for c in range(self.n_classes):
            name = class_names[c] if class_names else f"class {c}"
            for col, v in per[c].items():
                out[f"{name} {col}"] = v
        return out
