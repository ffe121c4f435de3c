"""Training crops over whole scenes (Model.train_scenes): RandLA-Net's training sampler (Hu et al., CVPR 2020; the authors'
spatially_regular_gen) with the scenes resident in HBM.  Every crop is the n nearest points (inside its scene) of the least
covered point over all scenes, whose "possibilities" then rise by (1 - d2/d2max)^2, as in Model.predict_scene; the crops
then go through the per-item preprocessing of the device loader (rl_batch_assemble: augmentation, collation).

Iterating yields what the device loader yields - (input (B,n,3+F) float32, labels (B,n) int64, scene (B,) int64), all on the
device - and the crop of a batch is decided on the device (rl_scenes_crop), so producing a batch never waits for the GPU.
Coordinates stay in the scene's own frame, the frame predict_scene feeds.

Host draws per crop, in this order: the centre noise (np.random.normal(0, center_noise, 3), only when center_noise > 0), then
the augmentation draws in the device loader's order (rng="numpy": jitter noise, scale, three angles, three shifts; rng="device":
the jitter noise comes from rl_batch_draw).  Torch's generator is not used.  The numpy twin of the crops is utils/scene.py
(scenes_crop).
"""
import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _hip as H
from .. import _ops as ops
from . import scene
from .augmentation import AugmentationSettings, _rotation
from .device_dataset import check_normal_column

Sample = Tuple[np.ndarray, np.ndarray, np.ndarray]
_RING = 4


def check_scenes(scenes: Sequence[Sample], n: int, pad_small_scenes: bool = False) -> int:
    """Validate (xyz (M,3), features (M,F), labels (M,)) scenes of at least n points - of at least one point with
    pad_small_scenes, which pads the crops of a smaller scene; returns F."""
    if len(scenes) == 0:
        raise ValueError("no scenes given")
    F = None
    for s, (xyz, features, labels) in enumerate(scenes):
        if xyz.ndim != 2 or xyz.shape[1] != 3:
            raise ValueError(f"scene {s}: xyz has shape {tuple(xyz.shape)}, expected (M, 3)")
        M = xyz.shape[0]
        if features.ndim != 2 or features.shape[0] != M:
            raise ValueError(f"scene {s}: features have shape {tuple(features.shape)}, expected ({M}, F)")
        if labels.shape != (M,):
            raise ValueError(f"scene {s}: labels have shape {tuple(labels.shape)}, expected ({M},)")
        if F is None:
            F = int(features.shape[1])
        if features.shape[1] != F:
            raise ValueError(f"scene {s}: {features.shape[1]} features, scene 0 has {F}")
        if M < (1 if pad_small_scenes else n):
            raise ValueError(f"scene {s} has {M} points, fewer than the crop size n={n}")
    if sum(x.shape[0] for x, _, _ in scenes) >= 2 ** 31 - 1:
        raise ValueError("the scenes hold 2^31 - 1 points or more")
    return F


def crop_draws(n: int, center_noise: float, aug: Optional[AugmentationSettings],
               jitter_on_host: bool) -> Tuple[np.ndarray, Optional[dict]]:
    """The host draws of one crop from numpy's global stream, in order: the centre noise (three normals, only when
    center_noise > 0; as float32), then - with augmentation - the device loader's draws: the jitter noise randn(n, 3) when it is
    drawn on the host, the scale, three angles, three shifts (augmentation.py's order).  Returns (centre (3,) float32, None or
    dict(jitter, scale, R, shift))."""
    centre = scene.centre_noise(center_noise)
    if not aug:
        return centre, None
    jitter = np.random.randn(n, 3) if jitter_on_host else None
    scale = np.random.uniform(1 - aug.scale_limit, 1 + aug.scale_limit)
    assert len(aug.rotation_angle_variances) == 3, "angle_sigmas should have length 3"
    assert len(aug.rotation_angle_limits) == 3, "angle_clips should have length 3"
    angles = [float(np.clip(s * np.random.randn(), -lim, lim))
              for s, lim in zip(aug.rotation_angle_variances, aug.rotation_angle_limits)]
    shift = np.random.uniform(-aug.shift_limit, aug.shift_limit, 3)
    return centre, dict(jitter=jitter, scale=scale, R=_rotation(*angles), shift=shift)


class SceneCropLoader:
    def __init__(self, scenes: Sequence[Sample], n: int, batch_size: int, crops_per_epoch: int, *,
                 center_noise: float = 0.0, augmentation_settings: Optional[AugmentationSettings] = None, seed: int = 0,
                 reset_each_epoch: bool = False, device=None, rng: str = "numpy", pad_small_scenes: bool = False,
                 normal_column: Optional[int] = None) -> None:
        if rng not in ("numpy", "device"):
            raise ValueError(f"rng must be 'numpy' or 'device', got {rng!r}")
        if n <= 0 or batch_size <= 0 or crops_per_epoch <= 0:
            raise ValueError(f"n={n}, batch_size={batch_size}, crops_per_epoch={crops_per_epoch}: all must be positive")
        self._F = check_scenes(scenes, n, pad_small_scenes)
        self._pad = bool(pad_small_scenes)
        self._normal_col = check_normal_column(normal_column, self._F)
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise H.HipKernelError("the scene crop loader needs a GPU: the crops are made on the device (rl_scenes_crop)")
        self.batch_size = int(batch_size)
        self.crops_per_epoch = int(crops_per_epoch)
        self.dataset = range(self.crops_per_epoch)          # (sized: the trainer reports its length)
        self.rng = rng
        self._n = int(n)
        self._noise_sigma = float(center_noise)
        self._aug = augmentation_settings
        self._reset = bool(reset_each_epoch)
        # device mode: rl_batch_draw's key, drawn like the device loader's (utils/device_dataset.py)
        self._seed = int(np.random.randint(0, 2 ** 31 - 1)) if rng == "device" else 0
        self._draws = 0
        sizes = [x.shape[0] for x, _, _ in scenes]
        self._S, self._max_points = len(sizes), max(sizes)
        dev = self.device
        # the scenes concatenated in HBM, float32 coordinates (converted once)
        self._xyz = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.float32) for x, _, _ in scenes])).to(dev)
        self._feat = torch.from_numpy(np.concatenate([np.asarray(f, dtype=np.float32).reshape(len(f), self._F)
                                                      for _, f, _ in scenes])).to(dev)
        self._lab = torch.from_numpy(np.concatenate([np.asarray(l).astype(np.int64) for _, _, l in scenes])).to(dev)
        self._off = torch.from_numpy(scene.scene_offsets(sizes)).to(dev)
        T = int(self._xyz.shape[0])
        poss = torch.from_numpy(scene.initial_possibility(T, seed)).to(dev)
        self._poss0 = poss.clone() if self._reset else None
        self.possibility = poss
        with torch.cuda.device(dev):
            self._ws = ops.scenes_workspace(dev, self._S, self._max_points, self._n)
            ops.scenes_init(self._off, self.possibility, self._ws, self._max_points)
        self._ring = None
        self._slot = 0
        self._checks = []            # (ring slot, error words, event) of the launched batches, oldest first

    def __len__(self) -> int:
        return (self.crops_per_epoch + self.batch_size - 1) // self.batch_size

    def _staging(self):
        """The next slot of a small ring of pinned host buffers (job records, centre noise, jitter noise in the numpy mode,
        the assemble launch's error words).  A slot is reused once the copies that last read it have run and its error
        words were looked at."""
        if self._ring is None:
            B, n = self.batch_size, self._n
            mk = lambda shape, dt: torch.empty(shape, dtype=dt).pin_memory()
            self._ring = [dict(jobs=mk((B * C.sizeof(H.CloudJob),), torch.uint8),
                               centre=mk((B, 3), torch.float32) if self._noise_sigma > 0 else None,
                               noise=mk((B, n, 3), torch.float64) if (self.rng == "numpy" and self._aug) else None,
                               words=mk((B,), torch.int32)) for _ in range(_RING)]
        k = self._slot
        self._slot = (k + 1) % _RING
        while self._checks and self._checks[0][0] == k:
            self._check_launches(wait=True, limit=1)
        return k, self._ring[k]

    def _job(self, job: H.CloudJob, aug: Optional[dict]) -> None:
        """The record of one crop: the concatenated arrays (the crop's rows are global), its augmentation draws."""
        job.xyz, job.features, job.labels = self._xyz.data_ptr(), self._feat.data_ptr(), self._lab.data_ptr()
        job.n_points, job.xyz_f64, job.normalization, job.augment = self._xyz.shape[0], 0, 0, 0
        job.normal_col = self._normal_col
        if aug is None:
            return
        job.augment = 1
        job.jitter_variance, job.jitter_limit = self._aug.jitter_variance, self._aug.jitter_limit
        job.scale = aug["scale"]
        for i in range(9):
            job.R[i] = float(aug["R"].flat[i])
        for i in range(3):
            job.shift[i] = float(aug["shift"][i])

    def _batch(self, B: int):
        """One batch on the CURRENT stream: host draws, staging copies, rl_scenes_crop, rl_batch_assemble."""
        n, F, dev = self._n, self._F, self.device
        stream = torch.cuda.current_stream(dev)
        k, st = self._staging()
        jobs = (H.CloudJob * B)()
        for b in range(B):
            centre, aug = crop_draws(n, self._noise_sigma, self._aug, jitter_on_host=st["noise"] is not None)
            if st["centre"] is not None:
                st["centre"].numpy()[b] = centre
            if st["noise"] is not None:
                st["noise"].numpy()[b] = aug["jitter"]
            self._job(jobs[b], aug)
        nbytes = B * C.sizeof(H.CloudJob)
        st["jobs"].numpy()[:nbytes] = np.frombuffer(bytes(jobs), dtype=np.uint8)
        jobs_dev = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        jobs_dev.copy_(st["jobs"][:nbytes], non_blocking=True)
        centre = None
        if st["centre"] is not None:
            centre = torch.empty((B, 3), dtype=torch.float32, device=dev)
            centre.copy_(st["centre"][:B], non_blocking=True)
        noise = None
        if self._aug:
            noise = torch.empty((B, n, 3), dtype=torch.float64, device=dev)
            if st["noise"] is not None:
                noise.copy_(st["noise"][:B], non_blocking=True)
        indices = torch.empty((B, n), dtype=torch.int64, device=dev)
        scenes = torch.empty(B, dtype=torch.int64, device=dev)
        ops.scenes_crop(self._xyz, self.possibility, n, indices, scenes, self._ws, self._S, self._max_points, centre,
                        pad=self._pad)
        if self.rng == "device" and noise is not None:
            self._draws += 1
            H.check(H.lib().rl_batch_draw(jobs_dev.data_ptr(), B, n, (self._seed << 32) | (self._draws & 0xFFFFFFFF),
                                          None, noise.data_ptr(), stream.cuda_stream), "rl_batch_draw")
        scratch = torch.empty(H.lib().rl_batch_assemble_scratch_doubles(B, n), dtype=torch.float64, device=dev)
        inp = torch.empty((B, n, 3 + F), dtype=torch.float32, device=dev)
        lab = torch.empty((B, n), dtype=torch.int64, device=dev)
        H.check(H.lib().rl_batch_assemble(jobs_dev.data_ptr(), B, n, F, indices.data_ptr(), H.ptr(noise),
                                          scratch.data_ptr(), inp.data_ptr(), lab.data_ptr(), stream.cuda_stream),
                "rl_batch_assemble")
        f0 = int(H.lib().rl_batch_assemble_flag_u32(B, n, 0))
        stride = int(H.lib().rl_batch_assemble_flag_u32(B, n, 1)) - f0 if B > 1 else 1
        words = st["words"][:B]
        words.copy_(scratch.view(torch.int32)[f0::stride][:B], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream)                         # (after the last copy that reads or writes the slot)
        self._checks.append((k, words, ev))
        self._check_launches(wait=False)
        return inp, lab, scenes

    def _check_launches(self, wait: bool, limit: Optional[int] = None) -> None:
        """Raise if a finished rl_batch_assemble launch reported a timed-out rendezvous.  wait=False: only launches whose
        error words have already arrived."""
        done = 0
        while self._checks and (limit is None or done < limit):
            _, words, ev = self._checks[0]
            if wait:
                ev.synchronize()
            elif not ev.query():
                return
            self._checks.pop(0)
            done += 1
            if bool((words & 2).any()):
                raise H.HipKernelError("rl_batch_assemble: normal_col does not fit the feature columns")
            if bool((words != 0).any()):
                raise H.HipKernelError("rl_batch_assemble: a cloud-wide rendezvous timed out (the launch was not "
                                       "co-resident: a CU mask or partition mode?)")

    def reset(self) -> None:
        """Possibilities back to their initial values (reset_each_epoch loaders), on the device."""
        with torch.cuda.device(self.device):
            self.possibility.copy_(self._poss0)
            ops.scenes_init(self._off, self.possibility, self._ws, self._max_points)

    def __iter__(self):
        if self._reset:
            self.reset()
        try:
            with torch.cuda.device(self.device):
                for start in range(0, self.crops_per_epoch, self.batch_size):
                    yield self._batch(min(self.batch_size, self.crops_per_epoch - start))
        finally:                                  # (also when the iteration stops early)
            self._check_launches(wait=True)


def get_scene_crop_loader(scenes: Sequence[Sample], n: int, batch_size: int, crops_per_epoch: int, *,
                          center_noise: float = 0.0, augmentation_settings: Optional[AugmentationSettings] = None,
                          seed: int = 0, reset_each_epoch: bool = False, device=None,
                          rng: str = "numpy", pad_small_scenes: bool = False,
                          normal_column: Optional[int] = None) -> SceneCropLoader:
    """A loader of `crops_per_epoch` crops of n points per epoch in batches of `batch_size` (the last one may be smaller).
    Possibilities start from np.random.default_rng(seed) and persist across epochs unless reset_each_epoch.
    pad_small_scenes: scenes of 1 .. n-1 points are accepted; a crop of one takes every point of the scene, raises each
    possibility once, and fills its n slots with the scene's rows repeated cyclically (rl_scenes_crop_padded; the authors
    draw the repeats with np.random.choice - utils/scene.py: padded_select says why this does not).  A repeated slot carries
    its point's features and label and its own augmentation jitter.
    normal_column: the first of three feature columns that hold a direction (a surface normal); the augmentation's rotation
    turns them with the crop (rl_cloud_job.normal_col)."""
    return SceneCropLoader(scenes, n, batch_size, crops_per_epoch, center_noise=center_noise,
                           augmentation_settings=augmentation_settings, seed=seed, reset_each_epoch=reset_each_epoch,
                           device=device, rng=rng, pad_small_scenes=pad_small_scenes, normal_column=normal_column)
