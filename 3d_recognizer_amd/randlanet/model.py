"""`Model`: the facade train.py / predict.py talk to (reference randlanet/model.py:21-336) -
construct, load / save (zip of `config` json + `model` state_dict, interchangeable with the
reference's files), predict (confidences), upsample, train, evaluate - on the MI355X kernels.  The pipeline behind the
scene methods (predict_scene and its kin) is _scene_path.py's; here are their signatures and what they do with a vote."""
import json
import logging
import os
import shutil
import tempfile
from collections import OrderedDict, namedtuple
from dataclasses import asdict
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _ops as ops
from ._hip import HipKernelError
from ._scene_path import ScenePath, VoteOptions, check_normals
from .utils.augmentation import AugmentationSettings
from .utils.losses import check_trainable_classes
from .utils.dataset import get_data_loader
from .utils.device_dataset import get_device_data_loader
from .utils.scene_loader import check_scenes, get_scene_crop_loader
from .utils.modules import RandLANet, RandLANetSettings, UpSampler
from .utils import boxes as box_utils
from .utils import cluster as cluster_utils
from .utils import depth as depth_utils
from .utils import grid as grid_utils
from .utils import keypoints as keypoint_utils
from .utils import planes as plane_utils
from .utils import registration as registration_utils
from .utils import scene
from .utils.preprocessing import sample_points
from .utils.trainer import Trainer, TrainingSettings

Sample = Tuple[np.ndarray, np.ndarray, np.ndarray]
InstanceResult = namedtuple("InstanceResult", ["instance", "label", "classes", "count", "centroid", "lo", "hi", "score"])
OrientedInstanceResult = namedtuple("OrientedInstanceResult", InstanceResult._fields + ("box_center", "box_axes", "box_extent",
                                                                                       "box_eigenvalues"))
ViewsPrediction = namedtuple("ViewsPrediction", ["confidences", "transformations", "fitness", "inlier_rmse", "status", "xyz"])


def _pick_device(use_gpu: bool) -> torch.device:
    return torch.device("cuda" if (torch.cuda.is_available() and use_gpu) else "cpu")


class Model:
    def __init__(self, settings: RandLANetSettings, weights: Optional[OrderedDict] = None, use_gpu: bool = True):
        self.device = _pick_device(use_gpu)
        self._model = RandLANet(settings, self.device)
        if weights is not None:
            self._model.load_state_dict(weights)
        self._model.eval()
        self._upsampler = UpSampler(settings.upsampling, self.device)
        self._scene_path = ScenePath(self._model, self.device)

    def __del__(self):
        try:
            torch.cuda.empty_cache()
        except AttributeError:
            pass

    def __str__(self) -> str:
        return str(self._model)

    @property
    def settings(self) -> RandLANetSettings:
        return self._model.settings

    @property
    def module(self) -> torch.nn.Module:
        return self._model

    # ------------------------------------------------------------------------- persistence
    @staticmethod
    def load(path: Path, use_gpu: bool = True, **kwargs) -> "Model":
        """Read a model zip (model.py:77-105); keyword arguments override stored settings."""
        path = Path(path)
        assert path.is_file(), f"Could not find model file at {path}!"
        device = _pick_device(use_gpu)
        with tempfile.TemporaryDirectory() as tmp:
            shutil.unpack_archive(str(path), tmp, format="zip")
            with open(os.path.join(tmp, "config")) as f:
                settings = RandLANetSettings(**json.load(f))
            state = torch.load(os.path.join(tmp, "model"), map_location=device)
        if "model" in state.keys():
            state = state["model"]
        settings.update(**kwargs)
        return Model(settings, weights=state, use_gpu=use_gpu)

    def save(self, path: Path) -> None:
        """Write `config` (json of the settings) + `model` (state_dict) as one zip at `path`."""
        path = Path(path)
        os.makedirs(path.parent, exist_ok=True)
        with tempfile.TemporaryDirectory() as payload, tempfile.TemporaryDirectory() as out:
            with open(os.path.join(payload, "config"), "w") as f:
                json.dump(asdict(self.settings), f)
            torch.save(self._model.state_dict(), os.path.join(payload, "model"))
            archive = shutil.make_archive(os.path.join(out, "file"), "zip", payload)
            shutil.move(archive, str(path))

    # --------------------------------------------------------------------------- inference
    def upsample(self, logits: torch.Tensor, xyz: torch.Tensor, xyz_upsampled: torch.Tensor) -> torch.Tensor:
        """Softmax confidences of `logits` (B,C,N1) carried to `xyz_upsampled` (B,N2,3) -> (B,C,N2)."""
        if self.device.type != "cuda":
            conf = torch.softmax(logits.to("cpu", torch.float32), dim=1)
        else:
            with torch.cuda.device(self.device):
                conf = ops.softmax_cf(logits.to(self.device, torch.float32).contiguous())
        return self._upsampler(conf.unsqueeze(3), xyz, xyz_upsampled).squeeze(-1)

    def _knn_advice(self) -> None:
        s = self.settings
        if s.n_points > 20000:
            if s.n_neighbors < 32:
                if s.knn != "kdtree":
                    logging.warning('For improved performance, it is recommended to use knn="kdtree" when '
                                    "N > 20000 and K < 32.")
            elif s.knn != "approximate":
                logging.warning('For improved performance, it is recommended to use knn="approximate" when '
                                "N > 20000 and K > 32.")
            if s.knn == "naive":
                logging.warning('Using knn="naive" for N > 20000 potentially has very low performance or '
                                "will reach an OOM!")
        elif s.knn != "naive":
            logging.warning('For improved performance, it is recommended to use knn="naive" when N < 20000.')

    def predict(self, xyz: np.ndarray, features: Optional[np.ndarray] = None,
                prepostprocess: bool = True) -> np.ndarray:
        """Class confidences (softmax) for one (N,3) or a batch (B,N,3) of clouds -> (C,N) / (B,C,N).
        With pre/post-processing the cloud is down-sampled to settings.n_points with the fixed seed 0
        and the confidences are carried back to every input point (model.py:146-235)."""
        self._knn_advice()          # the reference's messages; every choice runs the exact HIP search here
        assert xyz.shape[-1] == 3, "xyz should have shape (B) x N x 3!"
        batched = xyz.ndim != 2
        if not batched:
            xyz = xyz[None]
        if features is not None and features.ndim == 2:
            features = features[None]
        cloud = xyz
        if features is not None:
            assert xyz.shape[0] == features.shape[0], "xyz and features should have same batch size!"
            assert xyz.shape[1] == features.shape[1], "xyz and features should have same number of points!"
            cloud = np.concatenate((xyz, features), axis=-1)
        if self.settings.upsampling == "none":
            prepostprocess = False
        with torch.no_grad():
            full = torch.from_numpy(cloud.astype(np.float32))
            if prepostprocess:
                keep = sample_points(cloud.shape[1], self.settings.n_points, consistent=True)
                sampled = full[:, keep, :]
                logits = self._model(sampled.to(self._model.device))
                out = self.upsample(logits, sampled[:, :, :3], full[:, :, :3]).cpu().numpy()
            else:
                logits = self._model(full.to(self._model.device))
                # (the reference returns a device tensor in this branch, against its own annotation)
                if logits.is_cuda:
                    with torch.cuda.device(logits.device):
                        out = ops.softmax_cf(logits.contiguous()).cpu().numpy()
                else:
                    out = torch.softmax(logits, dim=1).numpy()
        return out if batched else out[0]

    def predict_depth(self, depth, camera: depth_utils.DepthCamera, *, temporal: Optional[depth_utils.TemporalFilter] = None,
                      z_range: Tuple[float, float] = (0.05, 0.6), stride: int = 1,
                      prepostprocess: bool = True) -> depth_utils.DepthPrediction:
        """Class confidences for the points of one depth frame (H, W) uint16 - what the reference's camera loop computes per
        frame (camera/realsense_camera.py:90-125, then Predictor.predict): utils/depth.py's depth_points - the temporal filter
        when `temporal` is given (it holds the state from frame to frame), the deprojection through `camera`, the pixels with
        z_lo < z < z_hi of every stride-th row and column - and then predict on that cloud.  Returns
        DepthPrediction(confidences (C, M), xyz (M, 3), pixel (M,) = v * W + u) as numpy arrays; its image(H, W) scatters the
        confidences back to the pixels.  The result equals predict(deproject_host(...).xyz) bit for bit.

        On a GPU-placed model the frame is uploaded (2 bytes per pixel) and the cloud is made on the device (csrc/depth.hip);
        M is read back, the sample of predict is drawn on the host - sample_points(M, n_points, consistent=True) - and gathered
        on the device, and the forward and the up-sampling read device tensors: the points visit the host only as part of the
        result.  A model placed on the CPU runs the numpy twin, then predict.  A frame without a pixel inside z_range raises
        ValueError; the refusals of utils/depth.py come before any work."""
        on_gpu = self.device.type == "cuda"
        cloud = depth_utils.depth_points(depth, camera, temporal, z_range, stride, device=self.device)
        if cloud.xyz.shape[0] == 0:
            raise ValueError("predict_depth: no pixel inside z_range")
        if not on_gpu:
            return depth_utils.DepthPrediction(self.predict(cloud.xyz, prepostprocess=prepostprocess), cloud.xyz, cloud.pixel)
        self._knn_advice()
        if self.settings.upsampling == "none":
            prepostprocess = False
        with torch.cuda.device(self.device), torch.no_grad():
            full = cloud.xyz[None]
            if prepostprocess:
                keep = sample_points(full.shape[1], self.settings.n_points, consistent=True)
                sampled = torch.index_select(full, 1, torch.from_numpy(keep).to(self.device))
                out = self.upsample(self._model(sampled), sampled, full)
            else:
                out = ops.softmax_cf(self._model(full).contiguous())
            return depth_utils.DepthPrediction(out[0].cpu().numpy(), cloud.xyz.cpu().numpy(), cloud.pixel.cpu().numpy())

    def predict_views(self, views: Sequence, *, icp: registration_utils.IcpSettings, to: str = "first", poses=None,
                      global_init: Optional[registration_utils.GlobalSettings] = None, return_global: bool = False,
                      **predict_scene_keywords) -> ViewsPrediction:
        """Class confidences for several overlapping views of one scene - a second depth camera, a handheld camera moving
        through a room, the stations of a terrestrial scan -, brought into the frame of view 0 by ICP (utils/registration.py)
        and voted on as ONE cloud.  views: a sequence of xyz (M_v, 3) or (xyz, features); all views carry features or none.
        View v > 0 is registered by registration.icp with the keywords of `icp` (an IcpSettings) and init = poses[v] when
        `poses` (a sequence of V (4, 4) transforms or None entries) gives one, otherwise the identity: with to="first" onto
        view 0; with to="previous" onto the already transformed view v-1, init then defaulting to that view's final
        transform - a moving camera.  The merged cloud is the concatenation of the views' `transformed` arrays in view order
        and goes to predict_scene with the remaining keywords (grid= is the way to thin the overlap; the return_* keywords
        are not taken).  Returns ViewsPrediction(confidences - a list of (C, M_v) arrays, the columns of the merged result
        split at the view boundaries -, transformations (V, 4, 4) float64, fitness (V,), inlier_rmse (V,), status - a list;
        view 0 has the identity, fitness 1, rmse 0 and status "reference" -, xyz (sum of M_v, 3) float32, the merged cloud:
        what predict_instances / predict_keypoints take).  It equals predict_scene(np.concatenate([views[0] xyz,
        icp(...).transformed, ...])) done by hand bit for bit.

        On a GPU-placed model the views are uploaded once, registered on the device (csrc/icp.hip, rl_knn_f32, rl_normals) and
        merged there; without features the merged cloud goes to predict_scene as a device tensor.  A model placed on the CPU
        runs the numpy twin, with the same bits.  The refusals of utils/registration.py and a view without points come before
        any work.

        global_init (a GlobalSettings; None: nothing below runs and no launch is added): a view v > 0 WITHOUT an entry in
        `poses` gets its initial pose from registration.global_registration between grid_subsample(view, cell=voxel) and the
        same of its target - view 0 with to="first", the already moved view v-1 with to="previous" -, with max_distance
        1.5 * voxel unless given, and the viewpoints of the two views (each view's own origin unless `viewpoints` gives one
        per view in that view's frame; the target's is carried into the target's frame).  ICP then runs on the full clouds
        exactly as above.  A global result whose status is not "refined" is not used: that view starts as it would have
        without global_init.  return_global=True: returns (ViewsPrediction, a list with every view's
        GlobalRegistrationResult, None where none was computed) instead.  On the GPU the subsampling, the descriptors
        (csrc/fpfh.hip), the matching (csrc/match.hip) and the RANSAC (csrc/global.hip) run on the device."""
        R = registration_utils
        gchk = None
        if global_init is not None:
            if not isinstance(global_init, R.GlobalSettings):
                raise ValueError(f"predict_views: global_init={global_init!r} must be a GlobalSettings")
            gchk = R.check_global_settings(global_init, len(views))
        if not isinstance(icp, R.IcpSettings):
            raise ValueError(f"predict_views: icp={icp!r} must be an IcpSettings")
        if to not in ("first", "previous"):
            raise ValueError(f"predict_views: to={to!r} must be 'first' or 'previous'")
        for name in ("return_counts", "return_outliers", "return_planes"):
            if predict_scene_keywords.get(name):
                raise ValueError(f"predict_views: {name} is not taken; call predict_scene on the merged xyz for it")
        pairs = [tuple(v) if isinstance(v, (tuple, list)) else (v, None) for v in views]
        V = len(pairs)
        if V < 1 or any(len(p) != 2 for p in pairs) or len({p[1] is None for p in pairs}) != 1:
            raise ValueError("predict_views: views must be a non-empty sequence of xyz or of (xyz, features), all of one kind")
        if poses is not None and len(poses) != V:
            raise ValueError(f"predict_views: poses has {len(poses)} entries for {V} views")
        settings = asdict(icp)
        max_distance = settings.pop("max_distance")
        inits = [None if poses is None or poses[v] is None else R.check_transform(poses[v], f"predict_views: poses[{v}]")
                 for v in range(V)]
        on_gpu = self.device.type == "cuda"
        clouds = [R._checked_cloud(x, f"views[{v}]", self.device, "predict_views") if on_gpu      # (a device tensor stays)
                  else R.check_cloud(R._host_array(x), f"views[{v}]", "predict_views") for v, (x, _) in enumerate(pairs)]
        features = None
        if pairs[0][1] is not None:
            for v, (_, f) in enumerate(pairs):
                if np.ndim(f) != 2 or np.shape(f)[0] != clouds[v].shape[0]:
                    raise ValueError(f"predict_views: features of view {v} have shape {np.shape(f)}, expected ({clouds[v].shape[0]}, F)")
            features = np.concatenate([np.asarray(f) for _, f in pairs], axis=0)
        T = np.tile(np.eye(4), (V, 1, 1))
        fitness, rmse, status = np.ones(V), np.zeros(V), ["reference"]
        if on_gpu:
            with torch.cuda.device(self.device):
                clouds = [c.to(self.device) for c in clouds]
        moved = [clouds[0]]
        found, thin = [None] * V, {}
        for v in range(1, V):
            init = inits[v] if inits[v] is not None else (T[v - 1] if to == "previous" else None)
            if gchk is not None and inits[v] is None:
                w = 0 if to == "first" else v - 1
                found[v] = R.global_between(clouds[v], moved[w], v, w, T[w], gchk, thin, self.device if on_gpu else None)
                if found[v].status == "refined":
                    init = found[v].transformation
            chk = R.check_parameters(max_distance, init=init, who="predict_views", **settings)
            target = moved[0] if to == "first" else moved[v - 1]
            if on_gpu:
                res = R.icp_device(clouds[v], target, None, chk, self.device, "predict_views")
            else:
                res = R.icp_host(clouds[v], target, max_distance=max_distance, init=init, **settings)
            T[v], fitness[v], rmse[v] = res.transformation, res.fitness, res.inlier_rmse
            status.append(res.status)
            moved.append(res.transformed)
        if on_gpu:
            with torch.cuda.device(self.device):
                merged = torch.cat(moved, dim=0)
            xyz = merged.cpu().numpy()
            out = self.predict_scene(merged if features is None else xyz, features, **predict_scene_keywords)
        else:
            xyz = np.concatenate(moved, axis=0)
            out = self.predict_scene(xyz, features, **predict_scene_keywords)
        bounds = np.cumsum([c.shape[0] for c in clouds])[:-1]
        res = ViewsPrediction([np.ascontiguousarray(p) for p in np.split(out, bounds, axis=1)], T, fitness, rmse, status, xyz)
        return (res, found) if return_global else res

    def predict_scene(self, xyz: np.ndarray, features: Optional[np.ndarray] = None, *, votes: int = 1,
                      batch_size: int = 8, smooth: float = 0.95, seed: int = 0, max_passes: Optional[int] = None,
                      return_counts: bool = False, grid: Optional[float] = None, pad_small_scenes: bool = False,
                      normals: Optional[int] = None, viewpoint=None, outliers: Optional[Tuple[int, float]] = None,
                      return_outliers: bool = False, remove_planes: Optional[plane_utils.PlaneRemoval] = None,
                      return_planes: bool = False):
        """Class confidences (C, M) for every point of one large scene (M, 3) (+ features (M, F)) by voted crops, the test
        protocol of RandLA-Net (Hu et al., CVPR 2020): each crop is the n = min(n_points, M) nearest points of the least
        covered point (its "possibility"), raised by (1 - d2/d2max)^2 afterwards; a pass is `batch_size` crops in order
        and one forward, which draws one np.random.permutation(n) as every forward does; each crop's softmax is blended
        into its points' probabilities, prob = smooth*prob + (1 - smooth)*softmax.  Passes run until every point was in
        `votes` crops.  Possibilities start from np.random.default_rng(seed).  Returns the probabilities normalised per
        point, and with return_counts the number of crops each point was in.  On an MI355X the crops, the blend and the
        coverage count stay on the device (csrc/scene.hip); a model placed on the CPU runs the numpy twin
        (utils/scene.py), crop for crop the same sequence.

        With `grid` (a cell edge, in the units of xyz) the scene is grid-subsampled first, as the authors do with every
        scan (utils/grid.py: one representative per occupied cell, barycentre and mean features; on a GPU-placed model by
        csrc/grid.hip, the sub-cloud never leaving the device).  The voted crops then run on the V representatives (M above
        reads V: n = min(n_points, V), possibilities from scene.initial_possibility(V, seed)), and raw point i receives the
        confidences - and with return_counts the count - of the representative of ITS OWN CELL, which lies within one cell
        edge of it on every axis.  This is deliberately not the authors' nearest-barycentre lookup: it is exact, needs no
        search over the raw points, and comes for free from the subsampling.

        With `pad_small_scenes` a scene of M < n_points points (V cells with `grid`) goes through the crops a large one does,
        the input train_scenes(pad_small_scenes=True) trains on: n = n_points, every crop is the whole scene - all
        possibilities raised once, T the largest d2 - its n slots holding point j mod M (rows 0 .. M-1, then repeated
        cyclically; rl_scene_crop_padded, utils/scene.py: padded_select), and only the first M slots of a crop's logits are
        blended and counted, so a point is voted once per crop.  One forward shape serves every scene, and scenes below
        the network's minimum size work.  This is deliberately not the authors' np.random.choice fill: cyclic repeats weigh
        every point the same within one repeat and add no random stream.  Scenes of n_points points or more are unaffected.

        With `normals` = k the four columns [n_x, n_y, n_z, curvature] of utils/normals.py (normal_features: every point's k
        nearest neighbours, the normal turned towards `viewpoint` - the sensor's position - or upward without one) are
        appended after the caller's features, so the model needs n_features = F + 4.  They are estimated after `grid`, on the
        representatives, where the density is uniform, and on the model's device: rl_knn_f32 + rl_normals on a GPU-placed
        model, the cloud never leaving the device; the numpy twin on a CPU-placed one, with the same bits.  A scene of fewer
        than k points (cells) raises ValueError.

        With `outliers` = (k, std_ratio) the statistical outliers of utils/outliers.py (PCL's StatisticalOutlierRemoval: a
        point whose mean distance to its k nearest neighbours lies more than std_ratio standard deviations above the cloud's
        mean of it - the flying pixels of a depth camera) are removed before anything else looks at the cloud: after `grid`,
        on the V representatives, where the density is uniform, and before `normals`, which are estimated on the V' kept
        points only, so no outlier lies in any neighbourhood.  Everything above then reads V' for M: n = min(n_points, V'),
        possibilities from scene.initial_possibility(V', seed), pad_small_scenes applies to V'.  A removed point - with `grid`
        every raw point of a removed representative's cell - receives an all-zero confidence column and count 0, and
        return_outliers appends the (M,) bool mask of the removed raw points as the last element of the returned tuple.  On a
        GPU-placed model rl_knn_f32 + csrc/outliers.hip, the cloud staying on the device from the grid through the filter to
        the votes; the numpy twin on a CPU-placed one, with the same bits.  A scene of fewer than k + 1 points (cells) raises
        ValueError.  Removed points are not given their nearest kept neighbour's vote, and predict_scenes, evaluate_* and
        train_scenes do not take the keyword: filter such scans with utils/outliers.py's remove_statistical_outliers.

        With `remove_planes` = PlaneRemoval(threshold, max_planes=1, min_points=3, iterations=1024, seed=0, axis=None,
        max_angle=None) the dominant planes of utils/planes.py's segment_planes (RANSAC, PCL's SACSegmentation: the desk under
        a hand, the ground, the floor and the walls) are taken out as well: after `grid` and `outliers`, on the kept
        representatives, and before `normals`, which are estimated on what is left.  Crops, possibilities, pad_small_scenes -
        and the clustering, boxes and keypoints of predict_instances / predict_keypoints - see the remaining cloud only.  A
        plane point - with `grid` every raw point of a removed cell - gets exactly what an outlier gets: an all-zero
        confidence column and count 0.  return_planes appends (planes (P, 4) float32 [nx, ny, nz, d], plane_id (M,) int32 per
        raw point, -1 for none) as the last element, after the outlier mask when both are asked for.  A cloud of fewer than 3
        points at that stage raises ValueError; when no plane is found nothing is removed.  On a GPU-placed model
        csrc/planes.hip, the cloud staying on the device; the numpy twin on a CPU-placed one, with the same bits.  Without the
        keyword nothing changes, the launches included.  predict_scenes, evaluate_* and train_scenes do not take it: filter
        such scans with utils/planes.py's remove_planes.

        On a GPU-placed model `xyz` may also be a float32 (M, 3) tensor on the model's device, with features=None - the cloud
        utils/depth.py's depth_points(..., device=model.device) makes from a depth frame: it is used where it lies, and the
        result equals that of the same call with xyz.cpu().numpy() bit for bit.  predict_keypoints takes one too; a tensor on
        another device or of another dtype, with features, with non-finite coordinates or on a CPU-placed model raises
        ValueError."""
        opt = VoteOptions(votes, batch_size, smooth, seed, max_passes, grid, pad_small_scenes, normals, viewpoint, outliers,
                          remove_planes)
        voted = self._scene_path.vote(xyz, features, opt, device_out=False)
        out, count, inverse = scene.normalise(voted.prob), voted.count, voted.inverse
        if inverse is not None:
            out, count = np.ascontiguousarray(out[:, inverse]), count[inverse]
            if opt.removing:            # (row -1 read the last kept point's column: overwritten here)
                removed = inverse < 0
                out[:, removed] = 0.0
                count[removed] = 0
        res = (out, count) if return_counts else (out,)
        if return_outliers:
            res += (np.zeros(xyz.shape[0], bool) if voted.outliers is None else voted.outliers,)
        if return_planes:
            res += (voted.planes_found(xyz.shape[0]),)
        return res if len(res) > 1 else res[0]

    def predict_instances(self, xyz: np.ndarray, features: Optional[np.ndarray] = None, *, radius: float,
                          min_points: int = 10, ignore_classes: Sequence[int] = (0,), min_confidence: float = 0.0,
                          votes: int = 1, batch_size: int = 8, smooth: float = 0.95, seed: int = 0,
                          max_passes: Optional[int] = None, grid: Optional[float] = None,
                          pad_small_scenes: bool = False, normals: Optional[int] = None,
                          viewpoint=None, oriented_boxes: bool = False, normal_angle: Optional[float] = None,
                          max_curvature: Optional[float] = None, cluster_normals: int = 16,
                          min_samples: int = 1, outliers: Optional[Tuple[int, float]] = None,
                          remove_planes: Optional[plane_utils.PlaneRemoval] = None,
                          return_planes: bool = False) -> InstanceResult:
        """The objects of one large scene (M, 3) (+ features (M, F)): the voted crops of predict_scene (the same keywords,
        the same crops), then per point the label - the argmax of its blended probabilities, ties to the lowest class - and
        its confidence, the label's share of them (utils/cluster.py: scene_labels; label -1 where the confidence is below
        `min_confidence`), then Euclidean clustering (utils/cluster.py: euclidean_clusters): points of the same label within
        `radius` of each other are joined, points labelled -1 or with a class in `ignore_classes` take no part, components of
        fewer than `min_points` points are dropped, and the kept ones are numbered by their smallest point index.  Returns
        InstanceResult(instance (M,) int32 - the instance of every point, -1 for none -, label (M,) int64, and per instance
        classes (I,) int64, count (I,) int32, centroid (I, 3), lo, hi (I, 3) - the bounding box - and score (I,) float32, the
        mean confidence of the members).  On an MI355X the probabilities never leave the device between the vote and the
        clustering (rl_scene_labels, csrc/cluster.hip); a model placed on the CPU runs the numpy twins, with the same result
        for the same probabilities.

        With `grid` the V representatives of the occupied cells are what is voted on, labelled and clustered: radius and
        min_points are in terms of them, and count, centroid, box and score are statistics over the representatives, not
        over the raw points.  `instance` and `label` are carried to every raw point from the representative of its own cell,
        as predict_scene carries the confidences.  `normals` and `viewpoint`: as in predict_scene.

        With `oriented_boxes` the result is an OrientedInstanceResult: the fields above, then per instance box_center (I, 3),
        box_axes (I, 3, 3) - row a is axis a, the longest first, right-handed -, box_extent (I, 3) and box_eigenvalues (I, 3)
        float32, the box along the principal axes of the instance's points (utils/boxes.py: instance_boxes over `instance`;
        csrc/boxes.hip on an MI355X, where the ids go from the clustering into the boxes without leaving the device).  They
        are always statistics over the RAW points, as `instance` is, also with `grid`.

        With `normal_angle` (degrees, inside (0, 90)) the clustering is smoothness-constrained (utils/cluster.py, "smooth
        edge"): two points are joined only if, besides, their surface normals lie within normal_angle of each other,
        whichever way each points, so the walls of a room, or a table top and the cabinet it stands against, come apart at
        the crease although they touch, while a smooth bend stays one object.  With `max_curvature` the points whose
        curvature (utils/normals.py: lambda_min / trace, 0 on a plane) is above it take no part and get instance -1: the
        points on the crease itself, whose estimated normal is a blend of the two surfaces.  max_curvature without
        normal_angle is a ValueError.  The normals and curvatures are those of the cloud that is clustered (with `grid` the
        representatives): with `normals` = k the four columns that were appended for the network, reused; otherwise they are
        estimated from `cluster_normals` neighbours and `viewpoint` for the clustering alone (a cloud of fewer points raises
        ValueError) - on a GPU-placed model by rl_knn_f32 + rl_normals, the cloud staying on the device from the vote to the
        instances, on a CPU-placed one by the numpy twin.  Without normal_angle nothing changes.

        With `min_samples` above 1 (an integer >= 1, else ValueError) the clustering is DBSCAN's (utils/cluster.py,
        "density"): a point is a core point when at least min_samples points of its label, itself included, lie within
        `radius` of it - whatever their normals -, only core points are joined and pass a component on, a point that is not
        core but within reach of a core point joins the nearest one's component (ties to the lowest index) and passes nothing
        on, and every other point gets instance -1.  A thread of stray points between two objects - mislabelled votes, the
        flying pixels of a depth camera - then no longer merges them.  min_points counts a component with its border points,
        and the numbering goes by the smallest core point.  With `grid` the count is in representatives.  On a GPU-placed
        model rl_cluster_union_dense; with min_samples = 1 nothing changes, the launches included.

        `outliers` = (k, std_ratio): as in predict_scene.  The removed points take no part in the votes, the normals or the
        clustering - radius, min_points, min_samples and the per-instance statistics see the V' kept points only - and get
        label -1 and instance -1; the fields of the result do not change.

        `remove_planes` = PlaneRemoval(...): as in predict_scene.  A plane point is treated exactly as an outlier is: it takes
        no part in the votes, the normals or the clustering and gets label -1 and instance -1, so two objects that stand on
        the same surface are no longer joined through it.  With return_planes the call returns (result, (planes (P, 4),
        plane_id (M,) int32 per raw point))."""
        opt = VoteOptions(votes, batch_size, smooth, seed, max_passes, grid, pad_small_scenes, normals, viewpoint, outliers,
                          remove_planes)
        res, _, box, voted = self._instances(xyz, features, radius, min_points, ignore_classes, min_confidence, opt,
                                             boxes=bool(oriented_boxes), normal_angle=normal_angle,
                                             max_curvature=max_curvature, cluster_normals=cluster_normals,
                                             min_samples=min_samples)
        if oriented_boxes:
            res = OrientedInstanceResult(*res, box.center, box.axes, box.extent, box.eigenvalues)
        return (res, voted.planes_found(xyz.shape[0])) if return_planes else res

    def _instances(self, xyz, features, radius, min_points, ignore_classes, min_confidence, opt: VoteOptions,
                   name="the scene", boxes=False, normal_angle=None, max_curvature=None, cluster_normals=16, min_samples=1):
        """predict_instances on one scene, voted on under `opt`.  Returns (InstanceResult, instance_d, boxes, the scene's
        Voted): on a GPU-placed model instance_d is the (M,) int32 device tensor `instance` was downloaded from (the raw
        points' one with `grid`), None otherwise; boxes is the BoxResult of utils/boxes.py over the raw points under
        `instance` when asked for, None otherwise."""
        normals, viewpoint = opt.normals, opt.viewpoint
        on_gpu = self.device.type == "cuda"
        instance_d, box = None, None
        # the clustering's own refusals come before the votes (the labels are checked as placeholders: they do not exist yet)
        cluster_utils.check_inputs(np.zeros((1, 3), np.float32), np.zeros(1, np.int64), radius, min_points, ignore_classes,
                                   None)
        min_samples = cluster_utils.check_min_samples(min_samples)
        smooth_rule = normal_angle is not None
        if max_curvature is not None and not smooth_rule:
            raise ValueError("predict_instances: max_curvature needs normal_angle")
        if smooth_rule:     # (normals and curvature are checked as placeholders too)
            _, cos_t, _, top = cluster_utils.check_smooth(1, np.zeros((1, 3), np.float32), normal_angle,
                                                          None if max_curvature is None else np.zeros(1, np.float32),
                                                          max_curvature)
            if normals is None:
                check_normals(cluster_normals, viewpoint)
        min_confidence = float(min_confidence)
        if np.isnan(min_confidence):
            raise ValueError("predict_instances: min_confidence is not a number")
        if not np.isfinite(np.asarray(xyz, dtype=np.float32)).all():
            raise ValueError("predict_instances: non-finite coordinates")
        voted = self._scene_path.vote(xyz, features, opt, device_out=on_gpu, name=name)
        prob, inverse, cloud, removing = voted.prob, voted.inverse, voted.cloud, opt.removing
        if on_gpu:
            with torch.cuda.device(self.device), torch.no_grad():
                pts = cloud if torch.is_tensor(cloud) else torch.from_numpy(cloud[:, :3]).to(self.device)
                pts = pts[:, :3].contiguous()
                label, conf = ops.scene_labels(prob, min_confidence)
                ignore = np.unique(np.asarray(tuple(ignore_classes), np.int64)).tolist()
                if smooth_rule:
                    nrm, curv = self._scene_path.cluster_normals(cloud, pts, normals, cluster_normals, viewpoint, name)
                    res = ops.smooth_clusters(pts, label, float(np.float32(radius)), nrm, float(cos_t), int(min_points),
                                              ignore, conf, curv if top is not None else None,
                                              float(top) if top is not None else None, min_samples=min_samples)
                else:
                    res = ops.euclidean_clusters(pts, label, float(np.float32(radius)), int(min_points), ignore, conf,
                                                 min_samples=min_samples)
                if inverse is not None:
                    inv = inverse.long()
                    res = (res[0][inv],) + tuple(res[1:])
                    label = label[inv]
                    if removing:                    # (row -1 read the last kept point: overwritten here)
                        res = (res[0].masked_fill(inv < 0, -1),) + tuple(res[1:])
                        label = label.masked_fill(inv < 0, -1)
                instance_d = res[0]
                if boxes and res[1].numel():
                    raw = pts if inverse is None else torch.from_numpy(
                        np.ascontiguousarray(np.asarray(xyz, dtype=np.float32))).to(self.device)
                    box = box_utils.BoxResult(*(t.cpu().numpy() for t in
                                                ops.instance_boxes(raw, instance_d.contiguous(), res[1].numel())))
                res = cluster_utils.ClusterResult(*(t.cpu().numpy() for t in res))
                label = label.cpu().numpy()
        else:
            label, conf = cluster_utils.scene_labels(prob, min_confidence)
            kw = {}
            if smooth_rule:
                nrm, curv = self._scene_path.cluster_normals(cloud, cloud[:, :3], normals, cluster_normals, viewpoint, name)
                kw = dict(normals=nrm, normal_angle=normal_angle)
                if max_curvature is not None:
                    kw.update(curvature=curv, max_curvature=max_curvature)
            res = cluster_utils.euclidean_clusters_host(cloud[:, :3], label, radius=radius, min_points=min_points,
                                                        ignore_classes=ignore_classes, scores=conf, min_samples=min_samples,
                                                        **kw)
            if inverse is not None:
                res = res._replace(instance=res.instance[inverse])
                label = label[inverse]
                if removing:
                    res.instance[inverse < 0] = -1
                    label[inverse < 0] = -1
            if boxes and res.count.shape[0]:
                box = box_utils.instance_boxes_host(xyz, res.instance, res.count.shape[0])
        if boxes and box is None:                   # no instance at all
            box = box_utils.instance_boxes_host(np.zeros((1, 3), np.float32), np.full(1, -1, np.int64))
        return InstanceResult(np.ascontiguousarray(res.instance), np.ascontiguousarray(label), *res[1:]), instance_d, box, voted

    def evaluate_instances(self, scenes: Sequence[tuple], class_names: Optional[List[str]] = None, *, radius: float,
                           min_points: int = 10, ignore_classes: Sequence[int] = (0,), min_confidence: float = 0.0,
                           min_gt_points: int = 1, iou_thresholds: Optional[Sequence[float]] = None, votes: int = 1,
                           batch_size: int = 8, smooth: float = 0.95, seed: int = 0, max_passes: Optional[int] = None,
                           grid: Optional[float] = None, pad_small_scenes: bool = False, normals: Optional[int] = None,
                           viewpoint=None, boxes: bool = False, normal_angle: Optional[float] = None,
                           max_curvature: Optional[float] = None, cluster_normals: int = 16, min_samples: int = 1):
        """Score predict_instances against annotated scenes (xyz (M,3), features (M,F) or None, labels (M,), instance_ids
        (M,)): every scene goes through exactly what predict_instances runs (the same keywords), and its predicted instances
        - per RAW point, also with `grid` - are matched against the ground-truth instances by utils/instance_metrics.py's
        InstanceEvaluator (ignore_classes, min_gt_points, iou_thresholds: see there; a point whose label is outside
        [0, n_classes) or ignored, or whose instance id is negative, belongs to no ground-truth instance).  Returns its
        result(): "AP" (mean over IoU 0.50 .. 0.95), "AP50", "AP25", "precision50", "recall50", "mCov", "mWCov" and the
        per-class entries, keyed by class_names when given.  On an MI355X the per-point instance ids go from the clustering
        into the pair counts (rl_pairs_*, csrc/pairs.hip) without leaving the device, and only the tables of pairs come
        back; a model placed on the CPU runs the numpy twins, with the same scores for the same predictions.  Wrong tuple
        lengths, labels or instance ids that are not (M,) integers and a class_names of the wrong length are ValueError
        before any vote.

        With `boxes` the result gains the detection scores of utils/box_metrics.py's BoxEvaluator - "box_AP25", "box_AP50"
        and their per-class entries, the ScanNet / SUN RGB-D box mAP - over axis-aligned boxes of the raw points: the
        predicted boxes from utils/boxes.py's instance_boxes under the predicted instances, the ground-truth boxes from
        the same function (on the model's device) under the scene's instance ids, masked as above; the class of a
        ground-truth box is its most frequent label, ties to the lowest.  Without it the result is unchanged.

        `normal_angle`, `max_curvature` and `cluster_normals`: the smoothness-constrained clustering of predict_instances, for
        every scene.  `min_samples`: its density rule, for every scene."""
        from .utils.box_metrics import BoxEvaluator
        from .utils.instance_metrics import InstanceEvaluator, pair_counts_host
        C = self.settings.n_classes
        if class_names is not None and len(class_names) != C:
            raise ValueError(f"evaluate_instances: {len(class_names)} class names for n_classes={C}")
        for k, sc in enumerate(scenes):
            if not isinstance(sc, (tuple, list)) or len(sc) != 4:
                raise ValueError(f"evaluate_instances: scene {k} is not a tuple (xyz, features, labels, instance_ids)")
            M = np.shape(sc[0])[0] if np.ndim(sc[0]) else 0
            for what, arr in (("labels", np.asarray(sc[2])), ("instance_ids", np.asarray(sc[3]))):
                if arr.shape != (M,) or arr.dtype.kind not in "iu":
                    raise ValueError(f"evaluate_instances: scene {k}: {what} have shape {tuple(arr.shape)} and dtype "
                                     f"{arr.dtype}, expected ({M},) integers")
        ev = InstanceEvaluator(C, ignore_classes=ignore_classes, min_gt_points=min_gt_points, iou_thresholds=iou_thresholds,
                               device=self.device)
        bev = BoxEvaluator(C, ignore_classes=ignore_classes, min_gt_points=min_gt_points) if boxes else None
        opt = VoteOptions(votes, batch_size, smooth, seed, max_passes, grid, pad_small_scenes, normals, viewpoint)
        for k, (xyz, features, labels, ids) in enumerate(scenes):
            res, instance_d, box, _ = self._instances(xyz, features, radius, min_points, ignore_classes, min_confidence, opt,
                                                      name=f"scene {k}", boxes=bool(boxes), normal_angle=normal_angle,
                                                      max_curvature=max_curvature, cluster_normals=cluster_normals,
                                                      min_samples=min_samples)
            ev.add(res.instance if instance_d is None else instance_d, res.classes, res.score, ids, labels)
            if boxes:
                gi, gl = np.asarray(ids).astype(np.int64), np.asarray(labels).astype(np.int64)
                valid = (gi >= 0) & (gl >= 0) & (gl < C) & ~np.isin(gl, ev.ignore)
                g1, l1 = np.where(valid, gi, -1), np.where(valid, gl, -1)
                n_gt = max(int(g1.max()) + 1, 1)
                gt = box_utils.instance_boxes(xyz, g1, n_gt, device=self.device)
                gt_class, most = np.full(n_gt, -1, np.int64), np.zeros(n_gt, np.int64)
                for g, l, n in zip(*(a.tolist() for a in pair_counts_host(g1, l1, n_gt, C))):
                    if g >= 0 and l >= 0 and n > most[g]:            # ascending (g, label): ties stay with the lowest
                        most[g], gt_class[g] = n, l
                bev.add(box.lo, box.hi, res.classes, res.score, gt.lo, gt.hi, gt_class, gt.count)
        out = ev.result(class_names)
        if boxes:
            out.update(bev.result(class_names))
        return out

    def predict_keypoints(self, xyz: np.ndarray, features: Optional[np.ndarray] = None, *, radius: float,
                          min_score: float = 0.5, min_points: int = 1, ignore_classes: Sequence[int] = (0,),
                          votes: int = 1, batch_size: int = 8, smooth: float = 0.95, seed: int = 0,
                          max_passes: Optional[int] = None, grid: Optional[float] = None, pad_small_scenes: bool = False,
                          normals: Optional[int] = None, viewpoint=None,
                          outliers: Optional[Tuple[int, float]] = None,
                          remove_planes: Optional[plane_utils.PlaneRemoval] = None,
                          return_planes: bool = False) -> keypoint_utils.KeypointResult:
        """The recognised points of one large scene (M, 3) (+ features (M, F)), one position and score each: the voted crops
        of predict_scene (the same keywords, the same crops), then per point the label and its confidence (utils/cluster.py:
        scene_labels), then the confidence peaks (utils/keypoints.py: confidence_peaks, whose docstring is the definition).  A
        point takes part when its class is not in `ignore_classes` and its confidence is at least `min_score`; it is live
        when at least `min_points` such points of its class lie within `radius` of it, itself included - a lone confident
        outlier is not -; a keypoint is a live point whose confidence no live point of its class within `radius` exceeds
        (equal confidences: the lowest index wins), so two keypoints of a class are more than `radius` apart, and two
        fingertips that touch stay two where predict_instances would merge them.  Returns KeypointResult(index (K,) int64 -
        the peak's point -, classes (K,) int64, position (K, 3) float32 - the confidence-weighted mean of the live points of
        the class within `radius` of the peak -, score (K,) float32 - the peak's confidence -, mean_score (K,) float32 and
        count (K,) int32 over those points), numbered in ascending index.  On an MI355X the probabilities never leave the
        device between the vote and the keypoints (rl_scene_labels, csrc/keypoints.hip); a model placed on the CPU runs the
        numpy twins, with the same result for the same probabilities.

        With `grid` the peaks are found on the V representatives of the occupied cells: radius, min_points and count are in
        terms of them, and `index` is the lowest raw point index whose cell is the peak's representative.  `normals` and
        `viewpoint`: as in predict_scene.  `outliers` = (k, std_ratio): as in predict_scene; a removed point is not a live
        point - it is no keypoint, supports none and drags no refined position.  `remove_planes` = PlaneRemoval(...): as in
        predict_scene; a plane point is treated exactly as an outlier is.  With return_planes the call returns (result,
        (planes (P, 4), plane_id (M,) int32 per raw point))."""
        opt = VoteOptions(votes, batch_size, smooth, seed, max_passes, grid, pad_small_scenes, normals, viewpoint, outliers,
                          remove_planes)
        res, voted = self._keypoints(xyz, features, radius, min_score, min_points, ignore_classes, opt)
        return (res, voted.planes_found(xyz.shape[0])) if return_planes else res

    def _keypoints(self, xyz, features, radius, min_score, min_points, ignore_classes, opt: VoteOptions, name="the scene"):
        """predict_keypoints on one scene, voted on under `opt`.  Returns (KeypointResult, the scene's Voted)."""
        on_gpu = self.device.type == "cuda"
        # the peaks' own refusals come before the votes (labels and scores are checked as placeholders: they do not exist yet)
        _, _, _, r, ms, min_points, ignore = keypoint_utils.check_inputs(
            np.zeros((1, 3), np.float32), np.zeros(1, np.int64), np.zeros(1, np.float32), radius, min_score, min_points,
            ignore_classes)
        # (a device tensor is checked on the device, by the scene path, before the first crop)
        if not torch.is_tensor(xyz) and not np.isfinite(np.asarray(xyz, dtype=np.float32)).all():
            raise ValueError("predict_keypoints: non-finite coordinates")
        voted = self._scene_path.vote(xyz, features, opt, device_out=on_gpu, name=name)
        prob, inverse, cloud, removing = voted.prob, voted.inverse, voted.cloud, opt.removing
        if on_gpu:
            with torch.cuda.device(self.device), torch.no_grad():
                pts = cloud if torch.is_tensor(cloud) else torch.from_numpy(cloud[:, :3]).to(self.device)
                pts = pts[:, :3].contiguous()
                label, conf = ops.scene_labels(prob)
                res = ops.confidence_peaks(pts, label, conf, float(r), float(ms), min_points, ignore.tolist())
                if inverse is not None:             # the lowest raw point of every cell, then of the peaks' cells
                    inv = inverse.long()
                    raw = torch.arange(inv.numel(), device=self.device)
                    if removing:                    # (the removed raw points have no row)
                        raw = raw[inv >= 0]
                        inv = inv[raw]
                    first = torch.full((pts.shape[0],), inverse.numel(), dtype=torch.int64, device=self.device)
                    first.scatter_reduce_(0, inv, raw, reduce="amin")
                    res = (first[res[0]],) + tuple(res[1:])
                res = keypoint_utils.KeypointResult(*(t.cpu().numpy() for t in res))
        else:
            label, conf = cluster_utils.scene_labels(prob)
            res = keypoint_utils.confidence_peaks_host(cloud[:, :3], label, conf, radius=radius, min_score=min_score,
                                                       min_points=min_points, ignore_classes=ignore_classes)
            if inverse is not None:
                first = np.full(cloud.shape[0], inverse.shape[0], np.int64)
                raw = np.arange(inverse.shape[0])
                if removing:                        # (the removed raw points have no row)
                    raw = raw[inverse >= 0]
                np.minimum.at(first, inverse[raw], raw)
                res = res._replace(index=first[res.index])
        return res, voted

    def evaluate_keypoints(self, scenes: Sequence[tuple], class_names: Optional[List[str]] = None, *, radius: float,
                           distances: Optional[Sequence[float]] = None, min_score: float = 0.5, min_points: int = 1,
                           ignore_classes: Sequence[int] = (0,), votes: int = 1, batch_size: int = 8, smooth: float = 0.95,
                           seed: int = 0, max_passes: Optional[int] = None, grid: Optional[float] = None,
                           pad_small_scenes: bool = False, normals: Optional[int] = None, viewpoint=None):
        """Score predict_keypoints against annotated scenes (xyz (M, 3), features (M, F) or None, keypoints (G, 3)[,
        keypoint_classes (G,)]) - without classes every annotated point is class 1; utils/keypoints.py's annotation_keypoints
        makes the positions from a per-point annotation mask.  Every scene goes through exactly what predict_keypoints runs
        (the same keywords), and its keypoints are matched against the annotated ones by utils/keypoint_metrics.py's
        KeypointEvaluator: per class and per distance in `distances` (default: half the radius, the radius and twice the
        radius), predictions in descending score take the nearest unmatched annotated point of their class within the
        distance.  Returns its result(): "precision@d", "recall@d", "F1@d", "AP@d" and "distance@d" (the mean distance of the
        matches) per distance, and the per-class entries, keyed by class_names when given.  Wrong tuple lengths, keypoints
        that are not (G, 3) and a class_names of the wrong length are ValueError before any vote."""
        from .utils.keypoint_metrics import KeypointEvaluator
        C = self.settings.n_classes
        if class_names is not None and len(class_names) != C:
            raise ValueError(f"evaluate_keypoints: {len(class_names)} class names for n_classes={C}")
        if distances is None:
            distances = (0.5 * float(radius), float(radius), 2.0 * float(radius))
        ev = KeypointEvaluator(C, distances, ignore_classes=ignore_classes)
        for k, sc in enumerate(scenes):
            if not isinstance(sc, (tuple, list)) or len(sc) not in (3, 4):
                raise ValueError(f"evaluate_keypoints: scene {k} is not a tuple (xyz, features, keypoints[, keypoint_classes])")
            kp = np.asarray(sc[2])
            if kp.size and (kp.ndim != 2 or kp.shape[1] != 3):
                raise ValueError(f"evaluate_keypoints: scene {k}: keypoints have shape {tuple(kp.shape)}, expected (G, 3)")
            if len(sc) == 4 and sc[3] is not None and np.shape(sc[3]) != (kp.reshape(-1, 3).shape[0],):
                raise ValueError(f"evaluate_keypoints: scene {k}: keypoint_classes have shape {np.shape(sc[3])}, expected "
                                 f"({kp.reshape(-1, 3).shape[0]},)")
        opt = VoteOptions(votes, batch_size, smooth, seed, max_passes, grid, pad_small_scenes, normals, viewpoint)
        for k, sc in enumerate(scenes):
            res, _ = self._keypoints(sc[0], sc[1], radius, min_score, min_points, ignore_classes, opt, name=f"scene {k}")
            ev.add(res.position, res.classes, res.score, sc[2], sc[3] if len(sc) == 4 else None)
        return ev.result(class_names)

    def predict_scenes(self, scenes: Sequence[tuple], *, votes: int = 1, batch_size: int = 8, smooth: float = 0.95,
                       seed: int = 0, max_passes: Optional[int] = None, return_counts: bool = False,
                       grid: Optional[float] = None, pad_small_scenes: bool = False,
                       max_resident_points: int = 2 ** 27, return_info: bool = False, normals: Optional[int] = None,
                       viewpoint=None):
        """predict_scene over many scenes at once: `scenes` is a sequence of (xyz (M,3), features (M,F) or None[, labels]),
        the result a list of (C, M_s) confidences, normalised as predict_scene's.  All scenes share the passes: every one of
        the `batch_size` crops of a pass goes to the least covered point among the scenes that still have a point in fewer
        than `votes` crops, and a scene leaves the competition the moment it is covered - a point's count rises when its crop
        is made, not when it is blended, so the next crop of the same pass already sees the scene closed.  A slot that finds
        no open scene is idle (its input rows stay what they were - zero before the first pass - and its logits are
        ignored).  Every scene's possibilities start from scene.initial_possibility(M_s, seed), and the crops taken from
        scene s are exactly the first crops predict_scene takes on s alone, up to the one that covers it; what is saved are
        the crops a scene-by-scene loop makes past that point to fill its last pass - with `pad_small_scenes` and votes=1
        a small scene costs one slot instead of one forward.  A pass is one forward (one np.random.permutation(n_points), as
        every forward draws); the blend always takes its softmax by the fixed exp (utils/scene.py: softmax_fixed), so GPU-
        and CPU-placed models blend the same bits from the same logits.  On an MI355X the crops, counts and blends stay on
        the device (rl_scenes_vote_crop, rl_scenes_vote_accumulate) and the host reads one integer per pass, the number of
        open scenes; a model placed on the CPU runs the numpy twin (utils/scene.py: scenes_vote_crop), crop for crop the
        same sequence.

        n is settings.n_points for every scene: a scene below it (after `grid`) raises ValueError naming the scene unless
        `pad_small_scenes` is set (padded crops as in predict_scene).  With `grid` every scene is grid-subsampled first and
        raw point i receives the column - and count - of its own cell's representative.  return_counts adds the list of
        per-scene counts, return_info a dict {"passes": the forwards run, "crops": the crops taken per scene (S,) int64}.

        Scenes are processed in consecutive groups whose total RAW points stay within `max_resident_points` (a single
        larger scene forms its own group); a group's scenes compete with each other only, and `max_passes` bounds the
        passes of each group (RuntimeError naming the scenes left uncovered).  A group keeps 4 * (3 + F + C + 3) bytes per
        (subsampled) point resident - cloud row, possibility, count, C probabilities, and the select keys of its largest
        scene - plus with `grid` 4 bytes per raw point for the cell of every point.

        `normals` and `viewpoint`: as in predict_scene, for every scene (one viewpoint for all; a scene of fewer than k
        points - cells, with `grid` - raises ValueError naming the scene)."""
        opt = VoteOptions(votes, batch_size, smooth, seed, max_passes, grid, pad_small_scenes, normals, viewpoint)
        probs, counts, crops, passes = [], [], [], 0
        for _, group, p, cr in self._scene_path.vote_together(scenes, opt, max_resident_points, device_out=False):
            passes += p
            crops.append(cr)
            for prob, count, inverse in group:
                out = scene.normalise(prob)
                if inverse is not None:
                    out, count = np.ascontiguousarray(out[:, inverse]), count[inverse]
                probs.append(out)
                counts.append(count)
        res = (probs,)
        if return_counts:
            res += (counts,)
        if return_info:
            res += ({"passes": passes, "crops": np.concatenate(crops) if crops else np.zeros(0, np.int64)},)
        return res if len(res) > 1 else probs

    def evaluate_scenes(self, scenes: Sequence[Sample], class_names: Optional[List[str]] = None, *,
                        grid: Optional[float] = None, votes: int = 1, batch_size: int = 8, smooth: float = 0.95,
                        seed: int = 0, max_passes: Optional[int] = None, return_confusion: bool = False,
                        pad_small_scenes: bool = False, together: bool = False,
                        max_resident_points: int = 2 ** 27, normals: Optional[int] = None, viewpoint=None):
        """Score whole scenes (xyz (M,3), features (M,F) or None, labels (M,)) of any size: every scene is predicted by the
        voted crops of predict_scene (the same keywords, `grid` and `pad_small_scenes` included - with the latter every scene
        runs at n_points, one forward shape for all, and the repeats of a padded crop are not counted) and all its RAW points, with their raw labels, are
        added to one confusion matrix over all scenes (row = label, column = argmax of the point's blended probabilities,
        ties to the lowest class; labels outside [0, n_classes) are unlabelled and skipped).  Returns "OA", "mAcc", "mIoU" and
        the per-class IoUs of that matrix (utils/grid.py: metrics_from_confusion; no "loss"), and the (C, C) int64 matrix as
        well with return_confusion.  On an MI355X the probabilities stay on the device and only the matrix comes back
        (rl_scene_confusion); a model placed on the CPU uses the numpy twins.

        With `together` the votes come from predict_scenes' path instead of the loop over the scenes: the scenes share the
        passes (n = n_points for every scene, groups bounded by `max_resident_points`), and each scene's slice of the
        probabilities goes through the same confusion count with its own cells.  A scene's crops are the first ones the
        loop takes on it; the forwards they ride in, and so the permutations, differ, and the blend takes the fixed exp.
        `normals` and `viewpoint`: as in predict_scene, for every scene."""
        opt = VoteOptions(votes, batch_size, smooth, seed, max_passes, grid, pad_small_scenes, normals, viewpoint)
        C = self.settings.n_classes
        assert class_names is None or len(class_names) == C, (
            "The length of given class names should correspond to the n_classes setting of the model")
        on_gpu = self.device.type == "cuda"
        conf = np.zeros((C, C), np.int64)
        table = torch.zeros((C, C), dtype=torch.int64, device=self.device) if on_gpu else None
        for k, (xyz, _, labels) in enumerate(scenes):
            assert np.shape(labels) == (xyz.shape[0],), \
                f"scene {k}: labels have shape {np.shape(labels)}, expected ({xyz.shape[0]},)"

        def voted():
            """(scene index, prob (V, C), inverse) of every scene, by either path"""
            if together:
                for k0, group, _, _ in self._scene_path.vote_together(scenes, opt, max_resident_points, device_out=on_gpu):
                    for j, (prob, _, inverse) in enumerate(group):
                        yield k0 + j, prob, inverse
            else:
                for k, (xyz, features, _) in enumerate(scenes):
                    voted = self._scene_path.vote(xyz, features, opt, device_out=on_gpu, name=f"scene {k}")
                    yield k, voted.prob, voted.inverse

        for k, prob, inverse in voted():
            labels = np.asarray(scenes[k][2])
            if on_gpu:
                with torch.cuda.device(self.device):
                    labels_d = torch.from_numpy(np.ascontiguousarray(labels.astype(np.int64))).to(self.device)
                    ops.scene_confusion(prob, labels_d, table, inverse)
            else:
                conf += grid_utils.confusion(prob, labels, C, inverse)
        if on_gpu:
            conf = table.cpu().numpy()
        out = grid_utils.metrics_from_confusion(conf, class_names)
        return (out, conf) if return_confusion else out

    # ---------------------------------------------------------------------------- training
    def _loader(self, dataset, n_points: int, batch_size: int, **kw):
        """get_data_loader (model.py:277-291, 326-332).  On a GPU the clouds live in HBM and every batch is assembled by
        one kernel (utils/device_dataset.py); the random numbers still come from numpy / torch in the reference's
        order unless RL_PIPELINE_RNG=device.  RL_HOST_PIPELINE=1 keeps the reference's host pipeline."""
        if self.device.type == "cuda" and not int(os.environ.get("RL_HOST_PIPELINE", "0")):
            return get_device_data_loader(dataset, n_points, batch_size, device=self.device,
                                          rng=os.environ.get("RL_PIPELINE_RNG", "numpy"), **kw)
        return get_data_loader(dataset, n_points, batch_size, **kw)

    def train(self, dataset_train: Sequence[Sample], dataset_validation: Sequence[Sample],
              training_settings: TrainingSettings = TrainingSettings(),
              augmentation_settings: AugmentationSettings = AugmentationSettings(),
              log_dir: Optional[Path] = None, class_names: Optional[List[str]] = None,
              callbacks: List[Callable[[int, Dict[str, float]], None]] = [], normal_column: Optional[int] = None):
        """Train from the current weights and keep the best ones (model.py:237-298).  With
        training_settings.ignore_unlabelled points labelled outside [0, n_classes) count nowhere - loss, gradients, training
        and validation metrics; training_settings.class_weights (which imply it) weight the labelled ones in the loss.
        normal_column: for clouds that bring their own normals - the first of three feature columns that hold a direction,
        which the augmentation's rotation then turns with the cloud (None: features are copied as they are)."""
        assert class_names is not None and len(class_names) == self.settings.n_classes, (
            "The length of given class names should correspond to the n_classes setting of the model")
        check_trainable_classes(self.settings.n_classes, "Model.train")
        n, bs = self.settings.n_points, training_settings.batch_size
        train_loader = self._loader(dataset_train, n, bs, shuffle=True, consistent_sampling=False,
                                    augmentation_settings=augmentation_settings, normal_column=normal_column)
        val_loader = self._loader(dataset_validation, n, bs, shuffle=False, consistent_sampling=True)
        trainer = Trainer(train_loader, val_loader, log_dir, class_names)
        self._model = self._scene_path.net = trainer.train(self._model, training_settings, callbacks=callbacks)

    def train_scenes(self, scenes_train: Sequence[Sample], scenes_validation: Sequence[Sample],
                     training_settings: TrainingSettings = TrainingSettings(),
                     augmentation_settings: AugmentationSettings = AugmentationSettings(), *, crops_per_epoch: int,
                     validation_crops: int, center_noise: float = 0.0, seed: int = 0, log_dir: Optional[Path] = None,
                     class_names: Optional[List[str]] = None,
                     callbacks: List[Callable[[int, Dict[str, float]], None]] = [], grid: Optional[float] = None,
                     pad_small_scenes: bool = False, normals: Optional[int] = None, viewpoint=None):
        """Train on whole scenes by spatial crops, RandLA-Net's training protocol and the crops predict_scene infers on: every
        crop is the n_points nearest points (inside its scene) of the least covered point over all scenes, offset by
        np.random.normal(0, center_noise, 3) when center_noise > 0.  An epoch is `crops_per_epoch` crops in batches of
        training_settings.batch_size; validation uses `validation_crops` crops of the validation scenes, from possibilities
        re-initialised before every pass (seed `seed`, no noise, no augmentation), so every epoch validates on the same crops.
        The Trainer is Model.train's.  Scenes are (xyz (M,3), features (M,F), labels (M,)) with M >= n_points.  GPU only:
        the crops are made on the device (utils/scene_loader.py).  With `grid` (a cell edge) every scene of both sets is
        grid-subsampled first (utils/grid.py: barycentres, mean features, majority labels over settings.n_classes), as the
        authors do with every scan; the scenes must hold n_points cells or more.
        Partly labelled scans: with training_settings.ignore_unlabelled (or class_weights, which imply it) labels outside
        [0, n_classes) are allowed - such a point counts nowhere in the loss, the gradients or the metrics, in a grid cell it
        does not vote, and a cell without a labelled point stays unlabelled (-1).  Without it they are refused by `grid` and
        count as before otherwise.
        With `pad_small_scenes` scenes of fewer than n_points points (cells, with `grid`) are accepted, as in the authors'
        generator: a crop of such a scene takes every point, raises each possibility once by (1 - d2/T)^2 (T the largest d2
        of the scene) and fills its n_points slots with the scene's rows repeated cyclically, slot j = row j mod M
        (rl_scenes_crop_padded; utils/scene.py: padded_select).  A repeated slot carries its point's features and label and
        counts in the loss and the crop metrics like any slot (an unlabelled point stays unlabelled); the augmentation jitter
        is per slot.  The authors draw the repeats with np.random.choice; cyclic repeats are a deliberate deviation - the
        device picks the scene, every point weighs the same within one repeat, and no new random stream enters the
        bitwise-reproducible training.  Pass the same keyword to predict_scene / evaluate_scenes.
        With `normals` = k every scene of both sets gets the four columns [n_x, n_y, n_z, curvature] of utils/normals.py
        appended after its F features (estimated after `grid`, on the cells; towards `viewpoint`, or upward without one; the
        model needs n_features = F + 4), and the augmentation's rotation turns the normal with every training crop
        (normal_column = F).  A scene of fewer than k points (cells) raises ValueError naming it.  Pass the same keywords to
        predict_scene / evaluate_scenes."""
        if self.device.type != "cuda":
            raise HipKernelError("train_scenes trains on the GPU (its crops are made by rl_scenes_crop): "
                                 "construct the Model with use_gpu=True on a machine with an MI355X")
        assert class_names is not None and len(class_names) == self.settings.n_classes, (
            "The length of given class names should correspond to the n_classes setting of the model")
        check_trainable_classes(self.settings.n_classes, "Model.train_scenes")
        n, bs = self.settings.n_points, training_settings.batch_size
        if grid is not None:
            allow = bool(training_settings.ignore_unlabelled) or training_settings.class_weights is not None
            scenes_train = self._grid_scenes(scenes_train, grid, allow)
            scenes_validation = self._grid_scenes(scenes_validation, grid, allow)
        normal_column = None
        if normals is not None:
            normal_column = check_scenes(scenes_train, 1)
            scenes_train = self._scene_path.normal_scenes(scenes_train, normals, viewpoint, "training")
            scenes_validation = self._scene_path.normal_scenes(scenes_validation, normals, viewpoint, "validation")
        rng = os.environ.get("RL_PIPELINE_RNG", "numpy")
        train_loader = get_scene_crop_loader(scenes_train, n, bs, crops_per_epoch, center_noise=center_noise,
                                             augmentation_settings=augmentation_settings, seed=seed, device=self.device,
                                             rng=rng, pad_small_scenes=pad_small_scenes, normal_column=normal_column)
        val_loader = get_scene_crop_loader(scenes_validation, n, bs, validation_crops, seed=seed, reset_each_epoch=True,
                                           device=self.device, pad_small_scenes=pad_small_scenes)
        trainer = Trainer(train_loader, val_loader, log_dir, class_names)
        self._model = self._scene_path.net = trainer.train(self._model, training_settings, callbacks=callbacks)

    def _grid_scenes(self, scenes: Sequence[Sample], cell: float, allow_unlabelled: bool = False) -> List[Sample]:
        """Every (xyz, features, labels) scene grid-subsampled on this model's device."""
        check_scenes(scenes, 1)
        out = []
        for xyz, features, labels in scenes:
            sub = grid_utils.grid_subsample(xyz, features, labels, cell=cell, n_classes=self.settings.n_classes,
                                            device=self.device, allow_unlabelled=allow_unlabelled)
            out.append((sub.xyz, sub.features, sub.labels))
        return out

    def evaluate(self, dataset: Sequence[Sample], class_names: Optional[List[str]] = None, batch_size: int = 16,
                 loss_function: str = "dice", postprocess: bool = False, include_stdev: bool = False,
                 class_weights: Optional[Sequence[float]] = None, ignore_unlabelled: bool = False) -> Dict:
        """class_weights / ignore_unlabelled: as in TrainingSettings - the loss and the metric counts over the labelled points."""
        check_trainable_classes(self.settings.n_classes, "Model.evaluate")
        loader = self._loader(dataset, self.settings.n_points, batch_size, shuffle=False, consistent_sampling=True)
        bag = Trainer.evaluate(self._model, loader, class_names, loss_function, postprocess, class_weights=class_weights,
                               ignore_unlabelled=ignore_unlabelled)
        return bag.as_dict(include_stdev=include_stdev)
