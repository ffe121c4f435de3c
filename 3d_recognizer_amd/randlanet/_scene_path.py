"""The scene pipeline behind Model.predict_scene and its kin: one scene -> grid-subsample -> remove outliers -> remove planes ->
append normals -> voted crops.  `VoteOptions` is what steers it, checked once per public call; `Voted` is what one scene's
vote returns; `ScenePath` runs it over a network and its device.  The public methods and their docstrings are Model's."""
from dataclasses import dataclass
from functools import cached_property
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _ops as ops
from .utils import grid as grid_utils
from .utils import normals as normal_utils
from .utils import outliers as outlier_utils
from .utils import planes as plane_utils
from .utils import scene

Sample = Tuple[np.ndarray, np.ndarray, np.ndarray]


def check_normals(normals, viewpoint) -> None:
    """The refusals of `normals` = k and `viewpoint` that do not depend on the scene (ValueError), before any work."""
    if normals is not None:
        normal_utils.check_inputs(np.zeros((normal_utils.MAX_K, 3), np.float32), normals, viewpoint)


def _check_outliers(outliers):
    """The refusals of `outliers` = (k, std_ratio) that do not depend on the scene (ValueError), before any work.  Returns
    (k as int, std_ratio as float), or None."""
    if outliers is None:
        return None
    if isinstance(outliers, (str, bytes)) or not hasattr(outliers, "__len__") or len(outliers) != 2:
        raise ValueError(f"outliers={outliers!r} must be a pair (k, std_ratio)")
    _, k, ratio = outlier_utils.check_inputs(np.zeros((outlier_utils.MAX_K + 1, 3), np.float32), outliers[0], outliers[1])
    return k, ratio


def _check_planes(remove_planes):
    """The refusals of `remove_planes` that do not depend on the scene (ValueError), before any work.  Returns the checked
    (threshold32, max_planes, min_points, T, axis32 or None, cos_min32), or None."""
    if remove_planes is None:
        return None
    if not isinstance(remove_planes, plane_utils.PlaneRemoval):
        raise ValueError(f"remove_planes={remove_planes!r} must be a PlaneRemoval")
    r = remove_planes
    np.random.default_rng(r.seed)               # (a seed the generator refuses raises here)
    return plane_utils.check_segmentation(r.threshold, r.max_planes, r.min_points, r.iterations, r.axis, r.max_angle,
                                          who="remove_planes")


@dataclass(frozen=True)
class VoteOptions:
    """The keywords the scene path shares (Model.predict_scene's docstring defines them; `pad` is pad_small_scenes), built
    once per public call, where votes / batch_size / smooth are refused (AssertionError).  The other refusals that do not
    depend on the scene are `checked`'s: they come where they always came, at the first vote, after the caller's own
    refusals and those of the scene's shape."""
    votes: int = 1
    batch_size: int = 8
    smooth: float = 0.95
    seed: int = 0
    max_passes: Optional[int] = None
    grid: Optional[float] = None
    pad: bool = False
    normals: Optional[int] = None
    viewpoint: object = None
    outliers: Optional[Tuple[int, float]] = None
    remove_planes: Optional[plane_utils.PlaneRemoval] = None

    def __post_init__(self):
        votes, batch_size, smooth = self.votes, self.batch_size, self.smooth
        assert votes >= 1 and batch_size >= 1 and 0.0 <= smooth < 1.0

    @cached_property
    def checked(self):
        """(outliers as (k, std_ratio), remove_planes as the arguments of plane_utils.check_segmentation), each None
        without its keyword, after the refusals (ValueError) of normals and viewpoint, outliers and remove_planes, in that
        order.  Kept on the record: the next scene of the same call checks nothing again."""
        check_normals(self.normals, self.viewpoint)
        return _check_outliers(self.outliers), _check_planes(self.remove_planes)

    @property
    def removing(self) -> bool:
        """Whether `inverse` can hold -1: a stage that removes points runs."""
        return self.outliers is not None or self.remove_planes is not None


class Voted(NamedTuple):
    """One scene's vote: prob (V, C) un-normalised and count (V,) over the V points the crops ran on; inverse (M,), the
    row of every raw point - None when the cloud was neither subsampled nor filtered, -1 for a removed point -; cloud (V,
    3 + F) float32, what the crops were taken from (a device tensor when a stage made it on the device, a numpy array
    otherwise); outliers, the (M,) bool mask of the raw points the outlier filter removed (None without the filter, and
    with device_out, where nobody reads it); planes, (planes (P, 4) float32 numpy, plane_id (M,) int32 per raw point), or
    None without remove_planes.  prob, count, inverse and plane_id are device tensors when device_out, numpy arrays
    otherwise."""
    prob: object
    count: object
    inverse: object
    V: int
    cloud: object
    outliers: object
    planes: Optional[tuple]

    def planes_found(self, M: int):
        """(planes (P, 4) float32, plane_id (M,) int32 per raw point) of return_planes, as numpy arrays."""
        if self.planes is None:
            return np.zeros((0, 4), np.float32), np.full(M, -1, np.int32)
        planes, pid = self.planes
        return planes, pid.cpu().numpy() if torch.is_tensor(pid) else pid


def _through(inverse, row):
    """row (V,) int32, a result per point of the cloud a stage saw, for every raw point: row[inverse], and -1 where
    `inverse` (M,) is -1 already (a point an earlier stage removed).  numpy arrays or device tensors, `row` itself without
    `inverse`."""
    if inverse is None:
        return row
    if torch.is_tensor(row):
        return torch.where(inverse >= 0, row[inverse.long().clamp(min=0)], torch.full_like(row[:1], -1))
    return np.where(inverse >= 0, row[np.maximum(inverse, 0)], -1).astype(np.int32)


class ScenePath:
    def __init__(self, net, device: torch.device):
        self.net, self.device = net, device

    @property
    def on_gpu(self) -> bool:
        return self.device.type == "cuda"

    def _device(self, a):
        """a numpy array, uploaded; a tensor already on the device stays where it is."""
        return a if torch.is_tensor(a) else torch.from_numpy(a).to(self.device)

    # ----------------------------------------------------------------------------------------------- votes
    def vote(self, xyz, features, opt: VoteOptions, *, device_out: bool, name: str = "the scene") -> Voted:
        """The voted crops of predict_scene over one scene: grid-subsampled first with opt.grid, then without its statistical
        outliers (opt.outliers), then without its planes (opt.remove_planes), then with the four columns of normal_features
        appended (opt.normals); a scene of fewer than n_points points runs padded crops of n_points slots with opt.pad.
        device_out (GPU models only): see Voted."""
        assert xyz.ndim == 2 and xyz.shape[1] == 3, "xyz should have shape N x 3!"
        if features is not None:
            assert features.ndim == 2 and features.shape[0] == xyz.shape[0], \
                "xyz and features should have same number of points!"
        s = self.net.settings
        outliers, planes = opt.checked
        mask = found = None
        cloud, inverse = self._scene_cloud(xyz, features, opt.grid, device_out, opt.normals)
        if outliers is not None:
            cloud, inverse = self.remove_outliers(cloud, inverse, outliers, device_out, name)
            if not device_out:
                mask = inverse < 0
        if planes is not None:
            cloud, inverse, found = self.remove_planes(cloud, inverse, planes, opt.remove_planes.seed, device_out, name)
        cloud = self.append_normals(cloud, opt.normals, opt.viewpoint, name)
        M, dim = cloud.shape
        assert dim == 3 + s.n_features, "Input should have shape (B, N, 3 + F)!"
        n = min(s.n_points, M)
        first = None                    # padded crops: the leading slots that are blended
        if opt.pad and M < s.n_points:
            assert M >= 1, "Input point cloud should have at least 1 point!"
            n, first = s.n_points, M
        assert n >= self.net._min_n_points, f"Input point cloud should have at least {self.net._min_n_points} points!"
        poss = scene.initial_possibility(M, opt.seed)
        if self.on_gpu:
            prob, count, passes = self._scene_passes_gpu(cloud, poss, n, opt, device_out=device_out, first=first)
        else:
            assert not device_out
            prob, count, passes = self._scene_passes_host(cloud, poss, n, opt, first=first)
        if passes is None:
            uncovered = int((count < opt.votes).sum())
            raise RuntimeError(f"predict_scene: {uncovered} of {M} points were in fewer than {opt.votes} crops after "
                               f"max_passes={opt.max_passes} passes")
        return Voted(prob, count, inverse, M, cloud, mask, found)

    def _scene_passes_host(self, cloud, poss, n, opt, first=None):
        """first: None, or M < n - every crop is the padded whole scene and its first M slots are blended."""
        B, votes, max_passes = opt.batch_size, opt.votes, opt.max_passes
        s32, oms32 = scene.blend_factors(opt.smooth)
        M, C = cloud.shape[0], self.net.settings.n_classes
        prob = np.zeros((M, C), np.float32)
        count = np.zeros(M, np.int32)
        rows = np.empty((B, n, cloud.shape[1]), np.float32)
        passes = 0
        while max_passes is None or passes < max_passes:
            idx = [scene.crop(cloud, poss, n, pad=first is not None) for _ in range(B)]
            for b in range(B):
                rows[b] = cloud[idx[b]]
            with torch.no_grad():
                logits = self.net(torch.from_numpy(rows)).numpy()
            for b in range(B):
                scene.accumulate(prob, count, logits[b], idx[b], oms32, s32, first)
            passes += 1
            if int(count.min()) >= votes:
                return prob, count, passes
        return prob, count, None

    def _scene_passes_gpu(self, cloud, poss, n, opt, device_out=False, first=None):
        """cloud (M, dim) float32: a numpy array, or a tensor already on the device.  prob and count come back as device
        tensors when device_out, as numpy arrays otherwise.  first: as in _scene_passes_host."""
        dev = self.device
        B, votes, max_passes = opt.batch_size, opt.votes, opt.max_passes
        s32, oms32 = scene.blend_factors(opt.smooth)
        M, C = cloud.shape[0], self.net.settings.n_classes
        with torch.cuda.device(dev), torch.no_grad():
            step = self.net.infer_step(B, n)
            cloud_d = self._device(cloud)
            poss_d = torch.from_numpy(poss).to(dev)
            prob = torch.zeros((M, C), dtype=torch.float32, device=dev)
            count = torch.zeros(M, dtype=torch.int32, device=dev)
            idx = torch.empty((B, n), dtype=torch.int32, device=dev)
            ws = ops.scene_workspace(dev, M, n)
            low = torch.empty(1, dtype=torch.int32, device=dev)
            passes, covered = 0, False
            while max_passes is None or passes < max_passes:
                for b in range(B):              # in order: each crop sees the possibilities the previous ones raised
                    ops.scene_crop(cloud_d, poss_d, n, step.inp[b], idx[b], ws, pad=first is not None)
                logits = step.step(np.random.permutation(n))
                for b in range(B):
                    ops.scene_accumulate(logits[b], idx[b], float(oms32), float(s32), prob, count, first)
                ops.scene_min_count(count, low, ws)
                passes += 1
                if int(low.item()) >= votes:    # the one read-back of a pass
                    covered = True
                    break
            if device_out:
                return prob, count, passes if covered else None
            return prob.cpu().numpy(), count.cpu().numpy(), passes if covered else None

    def vote_together(self, scenes, opt: VoteOptions, max_resident_points: int, *, device_out: bool):
        """The voted crops of predict_scenes, group by group.  Yields (index of the group's first scene, [(prob (V_s, C)
        un-normalised, count (V_s,), inverse (M_s,) or None without grid) per scene], passes, crops per scene (int64)) -
        device tensors when device_out (GPU models only), numpy arrays otherwise.  opt.outliers and opt.remove_planes are
        not taken."""
        s = self.net.settings
        n = s.n_points
        assert n >= self.net._min_n_points, f"n_points should be at least {self.net._min_n_points}!"
        assert max_resident_points >= 1
        opt.checked                     # (the refusals of normals and viewpoint)
        for k, sc in enumerate(scenes):
            xyz, features = sc[0], sc[1]
            assert xyz.ndim == 2 and xyz.shape[1] == 3, f"scene {k}: xyz should have shape N x 3!"
            assert xyz.shape[0] >= 1, f"scene {k}: a scene should have at least 1 point!"
            assert features is None or (features.ndim == 2 and features.shape[0] == xyz.shape[0]), \
                f"scene {k}: xyz and features should have same number of points!"
        zeroed = False
        k0 = 0
        while k0 < len(scenes):
            k1, total = k0 + 1, scenes[k0][0].shape[0]
            while k1 < len(scenes) and total + scenes[k1][0].shape[0] <= max_resident_points:
                total += scenes[k1][0].shape[0]
                k1 += 1
            clouds, inverses = [], []
            for k in range(k0, k1):
                cloud, inverse = self._scene_cloud(scenes[k][0], scenes[k][1], opt.grid, device_out, opt.normals)
                cloud = self.append_normals(cloud, opt.normals, opt.viewpoint, f"scene {k}")
                assert cloud.shape[1] == 3 + s.n_features, "Input should have shape (B, N, 3 + F)!"
                if cloud.shape[0] < n and not opt.pad:
                    raise ValueError(f"scene {k} has {cloud.shape[0]} points, fewer than the crop size n={n} "
                                     "(pass pad_small_scenes=True)")
                clouds.append(cloud)
                inverses.append(inverse)
            sizes = [int(c.shape[0]) for c in clouds]
            off = scene.scene_offsets(sizes)
            poss = np.concatenate([scene.initial_possibility(M, opt.seed) for M in sizes])
            run = self._scenes_passes_gpu if self.on_gpu else self._scenes_passes_host
            prob, count, passes, crops = run(clouds, off, poss, n, opt, not zeroed)
            zeroed = True
            if passes is None:
                cnt = count.cpu().numpy() if torch.is_tensor(count) else count
                left = [int(k0 + j) for j in np.flatnonzero(scene.scenes_low(off, cnt) < opt.votes)]
                raise RuntimeError(f"predict_scenes: scenes {left} have points in fewer than {opt.votes} crops after "
                                   f"max_passes={opt.max_passes} passes")
            if self.on_gpu and not device_out:
                prob, count = prob.cpu().numpy(), count.cpu().numpy()
            cut = [int(o) for o in off]
            group = [(prob[cut[j]:cut[j + 1]], count[cut[j]:cut[j + 1]], inverses[j]) for j in range(k1 - k0)]
            yield k0, group, passes, crops
            k0 = k1

    def _scenes_passes_host(self, clouds, off, poss, n, opt, zero_input):
        """One group of predict_scenes by the numpy twin.  Returns (prob (T, C), count (T,), passes or None when max_passes
        ran out, crops per scene)."""
        B, votes, max_passes, pad = opt.batch_size, opt.votes, opt.max_passes, opt.pad
        s32, oms32 = scene.blend_factors(opt.smooth)
        cloud = np.concatenate(clouds)
        S, C = len(clouds), self.net.settings.n_classes
        prob = np.zeros((cloud.shape[0], C), np.float32)
        count = np.zeros(cloud.shape[0], np.int32)
        crops = np.zeros(S, np.int64)
        rows = np.zeros((B, n, cloud.shape[1]), np.float32)       # (an idle slot of the first passes feeds zeros)
        passes = 0
        while max_passes is None or passes < max_passes:
            taken = [scene.scenes_vote_crop(cloud, off, poss, count, votes, n, pad) for _ in range(B)]
            for b, t in enumerate(taken):
                if t is not None:           # (an idle slot keeps the rows it held)
                    rows[b] = cloud[t[1]]
                    crops[t[0]] += 1
            with torch.no_grad():
                logits = self.net(torch.from_numpy(rows)).numpy()
            for b, t in enumerate(taken):
                if t is not None:
                    scene.scenes_vote_accumulate(prob, logits[b], t[1], oms32, s32, t[2])
            passes += 1
            if int(scene.scenes_low(off, count).min()) >= votes:
                return prob, count, passes, crops
        return prob, count, None, crops

    def _scenes_passes_gpu(self, clouds, off, poss, n, opt, zero_input):
        """One group of predict_scenes on the device: clouds are numpy arrays or device tensors.  Returns device tensors
        (prob (T, C), count (T,)), passes or None when max_passes ran out, and the crops per scene."""
        dev = self.device
        B, votes, max_passes, pad = opt.batch_size, opt.votes, opt.max_passes, opt.pad
        s32, oms32 = scene.blend_factors(opt.smooth)
        S, C, Mmax = len(clouds), self.net.settings.n_classes, int(np.diff(off).max())
        with torch.cuda.device(dev), torch.no_grad():
            step = self.net.infer_step(B, n)
            if zero_input:
                step.inp.zero_()            # an idle slot of the first passes feeds finite rows
            cloud = torch.cat([self._device(c) for c in clouds])
            T = cloud.shape[0]
            poss_d = torch.from_numpy(poss).to(dev)
            prob = torch.zeros((T, C), dtype=torch.float32, device=dev)
            count = torch.zeros(T, dtype=torch.int32, device=dev)
            low = torch.zeros(S, dtype=torch.int32, device=dev)
            idx = torch.empty((B, n), dtype=torch.int64, device=dev)
            taken = torch.empty(B, dtype=torch.int64, device=dev)
            first = torch.empty(B, dtype=torch.int32, device=dev)
            open_d = torch.empty(1, dtype=torch.int32, device=dev)
            ws = ops.scenes_workspace(dev, S, Mmax, n)
            ops.scenes_init(torch.from_numpy(off).to(dev), poss_d, ws, Mmax)
            log = []                        # the scene of every slot, read once at the end
            passes, covered = 0, False
            while max_passes is None or passes < max_passes:
                ops.scenes_vote_crop(cloud, poss_d, count, low, votes, n, step.inp, idx, taken, first, open_d, ws, S, Mmax,
                                     pad=pad)
                log.append(taken.clone())
                logits = step.step(np.random.permutation(n))
                ops.scenes_vote_accumulate(logits, idx, first, float(oms32), float(s32), prob)
                passes += 1
                if int(open_d.item()) == 0:     # the one read-back of a pass
                    covered = True
                    break
            took = torch.cat(log).cpu().numpy() if log else np.zeros(0, np.int64)
            crops = np.bincount(took[took >= 0], minlength=S).astype(np.int64)
        return prob, count, passes if covered else None, crops

    # ---------------------------------------------------------------------------------------------- stages
    def _scene_cloud(self, xyz, features, grid, device_out, normals=None):
        """One scene as the (V, 3 + F) float32 cloud the crops run on - a device tensor on a GPU-placed model with `grid`,
        a numpy array otherwise - and with `grid` the cell of every raw point (a device tensor when device_out).  normals
        (k or None): the four columns the caller appends afterwards are not in the cloud yet.  xyz may be a float32 (M, 3)
        tensor on this model's device (utils/depth.py's depth_points makes one), features then None: it stays there."""
        if torch.is_tensor(xyz):
            self._check_device_cloud(xyz, features)
            if grid is None:
                return xyz.contiguous(), None
            _, _, c = grid_utils.check_inputs(np.zeros((1, 3), np.float32), None, None, grid, None)
            assert self.net.settings.n_features == (4 if normals else 0), "Input should have shape (B, N, 3 + F)!"
            with torch.cuda.device(self.device), torch.no_grad():
                cloud, _, inverse, _ = ops.grid_subsample(xyz.contiguous(), None, float(c))
            return cloud, inverse if device_out else inverse.cpu().numpy()
        if grid is None:
            cloud = xyz if features is None else np.concatenate((xyz, features), axis=-1)
            return np.ascontiguousarray(cloud, dtype=np.float32), None
        if self.on_gpu:
            cloud, _, c = grid_utils.check_inputs(xyz, features, None, grid, None)
            assert cloud.shape[1] == 3 + self.net.settings.n_features - (4 if normals else 0), \
                "Input should have shape (B, N, 3 + F)!"
            with torch.cuda.device(self.device), torch.no_grad():
                cloud, _, inverse, _ = ops.grid_subsample(torch.from_numpy(cloud).to(self.device), None, float(c))
            return cloud, inverse if device_out else inverse.cpu().numpy()
        sub = grid_utils.grid_subsample_host(xyz, features, cell=grid)
        cloud = sub.xyz if sub.features is None else np.concatenate((sub.xyz, sub.features), axis=-1)
        return np.ascontiguousarray(cloud), sub.inverse

    def _check_device_cloud(self, xyz: torch.Tensor, features) -> None:
        """The refusals of a scene given as a device tensor, all ValueError, before any work on it: a model placed on the CPU,
        another device, another dtype or shape, features, no point or too many, non-finite coordinates (one reduction on the
        device and its read-back)."""
        if not self.on_gpu:
            raise ValueError("xyz is a tensor, but the model is placed on the CPU: pass a numpy array")
        index = torch.cuda.current_device() if self.device.index is None else self.device.index
        if not xyz.is_cuda or xyz.device.index != index:
            raise ValueError(f"xyz is a tensor on {xyz.device}, the model is on {self.device}")
        if xyz.dtype != torch.float32:
            raise ValueError(f"xyz is a {xyz.dtype} tensor, expected torch.float32")
        if features is not None:
            raise ValueError("features must be None with xyz as a device tensor")
        if xyz.dim() != 2 or xyz.shape[1] != 3 or not 1 <= xyz.shape[0] < grid_utils.MAX_POINTS:
            raise ValueError(f"xyz has shape {tuple(xyz.shape)}, expected (M, 3) with 1 <= M < 2^31 - 1")
        with torch.cuda.device(xyz.device):
            if not bool(torch.isfinite(xyz).all()):
                raise ValueError("xyz: non-finite coordinates")

    def remove_outliers(self, cloud, inverse, outliers, device_out, name: str):
        """cloud (V, 3 + F) float32 - a numpy array or a device tensor - without its statistical outliers (k, std_ratio),
        found on this model's device (a GPU-placed model returns a device tensor), and the kept row of every raw point, -1
        for a removed one: slot, or slot[inverse] with the cell `inverse` (M,) of every raw point - a device tensor when
        device_out, a numpy array otherwise."""
        k, ratio = outliers
        if cloud.shape[0] < k + 1:
            raise ValueError(f"{name} has {cloud.shape[0]} points, fewer than the k + 1 = {k + 1} neighbours of "
                             f"outliers=({k}, {ratio})")
        if not self.on_gpu:
            res = outlier_utils.statistical_outliers_host(cloud[:, :3], k, ratio)
            return np.ascontiguousarray(cloud[res.kept]), _through(inverse, res.slot)
        if not torch.is_tensor(cloud):       # (a cloud subsampled on the device had its coordinates checked before)
            outlier_utils.check_inputs(cloud[:, :3], k, ratio)
        with torch.cuda.device(self.device), torch.no_grad():
            cloud_d = self._device(cloud)
            _, slot, kept, _, _ = ops.statistical_outliers(cloud_d[:, :3].contiguous(), k, ratio)
            cloud_d = torch.index_select(cloud_d, 0, kept)
            slot = _through(None if inverse is None else self._device(inverse), slot)
            return cloud_d, slot if device_out else slot.cpu().numpy()

    def remove_planes(self, cloud, inverse, planes, seed, device_out, name: str):
        """cloud (V, 3 + F) float32 - a numpy array or a device tensor - without the planes of utils/planes.py's
        segment_planes (`planes`: the checked arguments of VoteOptions.checked), found on this model's device (a GPU-placed model
        returns a device tensor); the kept row of every raw point, -1 for a removed one - slot, or slot[inverse] where the
        row `inverse` (M,) of a raw point is not -1 already -; and (planes (P, 4) float32 numpy, plane_id per raw point
        int32).  The two per-point results are device tensors when device_out, numpy arrays otherwise."""
        thr32, P, mp, T, a32, cos_min = planes
        if cloud.shape[0] < 3:
            raise ValueError(f"{name} has {cloud.shape[0]} points, fewer than the 3 a plane of remove_planes needs")
        if not self.on_gpu:
            seg = plane_utils.segment_checked_host(plane_utils.check_cloud(cloud[:, :3], "remove_planes"), thr32, P, mp, T,
                                                   seed, a32, cos_min)
            return (np.ascontiguousarray(cloud[seg.kept]), _through(inverse, seg.slot),
                    (seg.planes, _through(inverse, seg.plane_id)))
        if not torch.is_tensor(cloud):       # (a cloud subsampled on the device had its coordinates checked before)
            plane_utils.check_cloud(cloud[:, :3], "remove_planes")
        with torch.cuda.device(self.device), torch.no_grad():
            cloud_d = self._device(cloud)
            found, _, pid, kept, slot = ops.segment_planes(cloud_d[:, :3].contiguous(), float(thr32), P, mp, T, seed, a32,
                                                           float(cos_min))
            cloud_d = torch.index_select(cloud_d, 0, kept)
            inv = None if inverse is None else self._device(inverse)
            slot, pid = _through(inv, slot), _through(inv, pid)
            if device_out:
                return cloud_d, slot, (found, pid)
            return cloud_d, slot.cpu().numpy(), (found, pid.cpu().numpy())

    def append_normals(self, cloud, k, viewpoint, name: str):
        """cloud (V, 3 + F) float32 - a numpy array or a device tensor - with the four columns of normal_features(k) appended,
        estimated on this model's device (a GPU-placed model returns a device tensor); k None: the cloud as it is."""
        if k is None:
            return cloud
        if cloud.shape[0] < k:
            raise ValueError(f"{name} has {cloud.shape[0]} points, fewer than the normals=k={k} neighbours of a normal")
        if not self.on_gpu:
            return np.ascontiguousarray(np.concatenate((cloud, normal_utils.normal_features(cloud[:, :3], k, viewpoint,
                                                                                            device="cpu")), axis=1))
        if not torch.is_tensor(cloud):       # (a cloud subsampled on the device had its coordinates checked before)
            _, _, viewpoint = normal_utils.check_inputs(cloud[:, :3], k, viewpoint)
        with torch.cuda.device(self.device), torch.no_grad():
            cloud_d = self._device(cloud)
            n, c = ops.estimate_normals(cloud_d[:, :3].contiguous(), int(k), viewpoint)
            return torch.cat((cloud_d, n, c[:, None]), dim=1).contiguous()

    def cluster_normals(self, cloud, pts, normals, k, viewpoint, name: str):
        """(normals (V, 3), curvature (V,)) float32 of the cloud that is clustered, for the smooth rule: the last four columns
        of `cloud` when `normals` appended them (append_normals), else estimated from k neighbours of pts (V, 3) on this
        model's device.  Device tensors when cloud or pts is one, numpy arrays otherwise."""
        if normals is not None:
            if torch.is_tensor(cloud):
                return cloud[:, -4:-1].contiguous(), cloud[:, -1].contiguous()
            return np.ascontiguousarray(cloud[:, -4:-1]), np.ascontiguousarray(cloud[:, -1])
        if pts.shape[0] < k:
            raise ValueError(f"{name} has {pts.shape[0]} points, fewer than the normals=k={k} neighbours of a normal")
        if torch.is_tensor(pts):
            return ops.estimate_normals(pts, int(k), viewpoint)
        return tuple(normal_utils.estimate_normals_host(pts, k, viewpoint))

    def normal_scenes(self, scenes: Sequence[Sample], k: int, viewpoint, what: str) -> List[Sample]:
        """Every (xyz, features, labels) scene with the four columns of normal_features(k) appended to its features, estimated
        on this model's device; a scene of fewer than k points raises ValueError naming it."""
        check_normals(k, viewpoint)
        out = []
        for j, (xyz, features, labels) in enumerate(scenes):
            if xyz.shape[0] < k:
                raise ValueError(f"{what} scene {j} has {xyz.shape[0]} points, fewer than the normals=k={k} neighbours "
                                 "of a normal")
            nf = normal_utils.normal_features(xyz, k, viewpoint, device=self.device)
            features = np.asarray(features, dtype=np.float32).reshape(xyz.shape[0], -1)
            out.append((xyz, np.ascontiguousarray(np.concatenate((features, nf), axis=1)), labels))
        return out
