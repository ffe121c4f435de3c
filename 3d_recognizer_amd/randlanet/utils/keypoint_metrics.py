"""Scores of predicted keypoints against annotated ones: distances between points, where utils/instance_metrics.py scores
overlaps between point sets.  Host code, float64, small: a scene has a handful of keypoints.

  per class and per distance threshold d, over all scenes added so far:
  order       the predictions of the class in descending score; ties by scene (the order of add), then by keypoint number
  match       each prediction, in that order, takes the nearest still-unmatched ground-truth point of its class in its own
              scene whose Euclidean distance (float64) is <= d; ties to the lowest ground-truth index.  A ground-truth point
              is matched once: a second prediction on it is a false positive, as is a prediction of the wrong class
  scores      precision = TP / predictions, recall = TP / ground-truth points, F1 their harmonic mean (0 when both are 0), AP
              the area under the precision envelope of the ordered predictions - utils/instance_metrics.py's
              average_precision, the same integration as the instance AP -, and distance, the mean distance of the matches.
              NaN where the denominator is empty: precision without predictions, recall and AP without ground truth,
              distance without matches

Matches never cross scenes, and the order inside a scene is the global order restricted to it, so a scene is matched when it
is added.  The keypoints may come from Model.predict_keypoints, confidence_peaks or any other means."""
from collections import OrderedDict

import numpy as np

from .instance_metrics import _mean, average_precision


def _label(d: float) -> str:
    return f"{d:g}"


class KeypointEvaluator:
    """Accumulates scenes (add) and scores them (result); see the module docstring for the protocol."""

    def __init__(self, n_classes: int, distances, *, ignore_classes=(0,)):
        if int(n_classes) != n_classes or int(n_classes) < 1:
            raise ValueError(f"KeypointEvaluator: n_classes={n_classes!r} must be an integer >= 1")
        self.n_classes = int(n_classes)
        try:
            dist = tuple(float(d) for d in distances)
        except TypeError:
            dist = ()
        if not dist or any(not (np.isfinite(d) and d >= 0.0) for d in dist) or len(set(dist)) != len(dist):
            raise ValueError(f"KeypointEvaluator: distances={distances!r} must be distinct finite numbers >= 0")
        self.distances = dist
        ignore = np.asarray(tuple(ignore_classes) if ignore_classes is not None else (), dtype=np.int64)
        if ignore.ndim != 1:
            raise ValueError(f"KeypointEvaluator: ignore_classes has shape {tuple(ignore.shape)}, expected a flat sequence")
        self.ignore = np.unique(ignore)
        self.classes = [c for c in range(self.n_classes) if c not in set(self.ignore.tolist())]
        self.scenes = 0
        self.n_gt = {c: 0 for c in self.classes}
        self.n_pred = {c: 0 for c in self.classes}
        # per (class, distance): (score, scene, keypoint number, matched, distance of the match)
        self.rows = {(c, d): [] for c in self.classes for d in self.distances}

    def add(self, pred_position, pred_classes, pred_scores, gt_position, gt_classes=None) -> None:
        """One scene: pred_position (K, 3), pred_classes (K,) integers and pred_scores (K,) of the predicted keypoints;
        gt_position (G, 3) and gt_classes (G,) integers of the annotated ones - without classes every one is class 1.
        Refusals are ValueError."""
        pp = np.asarray(pred_position, dtype=np.float64).reshape(-1, 3) if np.size(pred_position) == 0 else \
            np.asarray(pred_position, dtype=np.float64)
        gp = np.asarray(gt_position, dtype=np.float64).reshape(-1, 3) if np.size(gt_position) == 0 else \
            np.asarray(gt_position, dtype=np.float64)
        for what, a in (("pred_position", pp), ("gt_position", gp)):
            if a.ndim != 2 or a.shape[1] != 3 or not np.isfinite(a).all():
                raise ValueError(f"KeypointEvaluator.add: {what} has shape {tuple(a.shape)}, expected finite (n, 3)")
        Kn, Gn = pp.shape[0], gp.shape[0]
        pc = np.asarray(pred_classes)
        if pc.shape != (Kn,) or (Kn and pc.dtype.kind not in "iu"):
            raise ValueError(f"KeypointEvaluator.add: pred_classes have shape {tuple(pc.shape)} and dtype {pc.dtype}, "
                             f"expected ({Kn},) integers")
        ps = np.asarray(pred_scores, dtype=np.float64)
        if ps.shape != (Kn,) or np.isnan(ps).any():
            raise ValueError(f"KeypointEvaluator.add: pred_scores have shape {tuple(ps.shape)}, expected ({Kn},) numbers")
        gc = np.ones(Gn, np.int64) if gt_classes is None else np.asarray(gt_classes)
        if gc.shape != (Gn,) or (Gn and gc.dtype.kind not in "iu"):
            raise ValueError(f"KeypointEvaluator.add: gt_classes have shape {tuple(gc.shape)} and dtype {gc.dtype}, "
                             f"expected ({Gn},) integers")
        pc, gc = pc.astype(np.int64), gc.astype(np.int64)
        scene = self.scenes
        self.scenes += 1
        for c in self.classes:
            preds = sorted(np.flatnonzero(pc == c).tolist(), key=lambda p: (-ps[p], p))
            gts = np.flatnonzero(gc == c)
            self.n_pred[c] += len(preds)
            self.n_gt[c] += gts.size
            diff = pp[preds][:, None, :] - gp[gts][None, :, :]
            dist = np.sqrt((diff * diff).sum(axis=2))                  # (predictions in order, ground truth ascending)
            for d in self.distances:
                free = np.ones(gts.size, bool)
                rows = self.rows[(c, d)]
                for n, p in enumerate(preds):
                    ok = free & (dist[n] <= d)
                    if ok.any():
                        g = int(np.argmin(np.where(ok, dist[n], np.inf)))   # the first minimum: the lowest index
                        free[g] = False
                        rows.append((ps[p], scene, p, True, float(dist[n, g])))
                    else:
                        rows.append((ps[p], scene, p, False, float("nan")))

    def result(self, class_names=None) -> OrderedDict:
        """Per distance d (written as "%g"): "precision@d", "recall@d", "F1@d", "AP@d" and "distance@d" - each the mean over
        the classes, NaN skipped -, then per class "<class> precision@d" ... and "<class> n_gt", "<class> n_pred" ("class
        c" without names; an ignored class has NaN scores and zero counts)."""
        if class_names is not None and len(class_names) != self.n_classes:
            raise ValueError(f"KeypointEvaluator.result: {len(class_names)} class names for n_classes={self.n_classes}")
        nan = float("nan")
        cols = ("precision", "recall", "F1", "AP", "distance")
        per = {}
        for c in range(self.n_classes):
            per[c] = {f"{col}@{_label(d)}": nan for d in self.distances for col in cols}
            per[c].update(n_gt=self.n_gt.get(c, 0), n_pred=self.n_pred.get(c, 0))
            if c not in self.n_gt:
                continue
            n_gt = self.n_gt[c]
            for d in self.distances:
                rows = sorted(self.rows[(c, d)], key=lambda r: (-r[0], r[1], r[2]))
                tp = np.array([r[3] for r in rows], dtype=bool)
                n_tp = int(tp.sum())
                precision = n_tp / tp.shape[0] if tp.shape[0] else nan
                recall = n_tp / n_gt if n_gt else nan
                f1 = nan if np.isnan(precision) or np.isnan(recall) else \
                    (2.0 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0)
                mean_d = float(np.mean([r[4] for r in rows if r[3]])) if n_tp else nan
                for col, v in zip(cols, (precision, recall, f1, average_precision(tp, n_gt), mean_d)):
                    per[c][f"{col}@{_label(d)}"] = v
        out = OrderedDict()
        for d in self.distances:
            for col in cols:
                key = f"{col}@{_label(d)}"
                out[key] = _mean([per[c][key] for c in range(self.n_classes)])
        for c in range(self.n_classes):
            name = class_names[c] if class_names else f"class {c}"
            for key, v in per[c].items():
                out[f"{name} {key}"] = v
        return out
