"""TSDF fusion of a stream of depth frames: what a camera that keeps delivering frames needs between utils/depth.py (one frame
to points) and the scene path (votes on a cloud).  Every frame is integrated into a dense truncated signed distance volume
(KinectFusion; Open3D's TSDFVolume), the next frame is registered against the surface of that volume (frame to model, by
utils/registration.py's ICP), and the surface is read out as points.  Sensor noise is averaged instead of kept, a surface seen
twice stays one surface, the cloud does not grow with the number of frames, and the drift of frame-to-frame registration does
not accumulate.

This module is the numpy host twin of csrc/tsdf.hip (include/rl_randlanet.h, rl_tsdf_*) and the public TsdfVolume / DepthFusion.
The twin's arithmetic is the specification; the kernels equal it bit for bit.  All arithmetic is float32, one correctly rounded
operation at a time, in the order written here; nothing is fused; division is true division:

  volume         TsdfVolume(origin, voxel, dims, trunc=None, max_weight=64, device=None).  origin = (ox, oy, oz), the minimum
                 corner, float32; voxel the edge length; dims = (nx, ny, nz); trunc defaults to float32(4) * voxel; max_weight
                 an integer in 1 .. 65535.  The state is two arrays of shape (nz, ny, nx), x fastest: tsdf float32, all 1.0 at
                 the start, and weight float32, all 0.0 - numpy arrays on the host path, device tensors on the device path (the
                 device is `device`, else cuda when there is one).  reset() restores the start.  Voxel (i, j, k) has the linear
                 index n = (k*ny + j)*nx + i and the centre c_x = ox + (float32(i) + 0.5) * voxel - add, multiply, add -,
                 likewise c_y, c_z
  pose           integrate(depth, camera, pose=None, z_range=(0.05, 0.6)): pose is the (4, 4) camera-to-world transform (None:
                 the identity), checked by registration.check_transform.  world_to_camera(pose) makes twelve floats on the host
                 in float64 - R' = R^T, t' = -(R^T t) - and rounds them to float32 once, R' row-major and then t'; both paths
                 use these same twelve floats
  integrate      per voxel:  q_a = ((R'_a0*c_x + R'_a1*c_y) + R'_a2*c_z) + t'_a for a = x, y, z (rl_icp_transform's rule); skip
                 unless q_z > 0; uf = ((q_x / q_z) * fx + ppx) + 0.5 and vf = ((q_y / q_z) * fy + ppy) + 0.5; skip unless
                 uf >= 0 and uf < float32(W) and vf >= 0 and vf < float32(H) (a NaN or an infinity skips; tested before any
                 conversion to an integer); u = int(uf), v = int(vf) - truncation, which is the nearest pixel -; d = depth[v, u];
                 skip if d == 0; z = float32(d) * depth_scale; skip unless z_lo < z and z < z_hi (both strict, as in deproject);
                 sdf = z - q_z, the projective distance along the camera's z axis; skip if sdf < -trunc; s = sdf / trunc, and 1
                 where that exceeds 1; with the voxel's old weight w: tsdf = (tsdf * w + s) / (w + 1), then
                 weight = min(w + 1, max_weight).  A skipped voxel is not written
  depth          (H, W) uint16, a numpy array or a device tensor, checked by depth.check_frame; W and H below 2^24.  A camera
                 with coeffs is refused: the inverse Brown-Conrady model is closed form only in the deprojecting direction.  A
                 caller who wants the temporal filter passes TemporalFilter.process(frame)
  extract        extract(min_weight=1) -> TsdfCloud(xyz (M, 3) float32, edge (M,) int64).  Voxels n ascending, inside each the
                 axes a = 0, 1, 2 (x, y, z) in that order; the neighbour b is one step up along a, if it lies inside the volume.
                 The edge emits a point when weight[n] >= min_weight and weight[b] >= min_weight and
                 (tsdf[n] < 0) != (tsdf[b] < 0).  Then f = tsdf[n] / (tsdf[n] - tsdf[b]) and the point is the centre of n with
                 coordinate a replaced by c_a + f * voxel (the product rounded, then added); edge = 3n + a, ascending by
                 construction.  M = 0 is a valid result with empty arrays.  min_weight: an integer in 1 .. max_weight
  refusals       all ValueError, before any work: voxel or trunc not finite and greater than 0; a dim below 1, or nx*ny*nz >=
                 2^31; max_weight or min_weight out of range; a frame of the wrong dtype or shape for the camera, or W or H of
                 2^24 or more; z_lo >= z_hi; a camera with coeffs; a pose that check_transform refuses

DepthFusion(model, camera, volume, icp=None, temporal=None, ...) is the camera loop around it: add(frame) tracks the frame
against the volume's surface and integrates it, predict() votes on the surface with model.predict_scene.

Not here: voxel hashing or sparse volumes, ray casting, normals from the TSDF gradient (normals=k of the scene path estimates
them), colour or per-class probabilities in the voxels, meshing, per-pixel weights, distorted cameras.
"""
from collections import namedtuple
from dataclasses import asdict

import numpy as np

from . import depth as D
from . import registration as R

_F32 = np.float32
MAX_VOXELS = 2 ** 31
MIN_WEIGHT, MAX_WEIGHT = 1, 65535
MAX_SIDE = 2 ** 24                       # W and H below it: float32(W) is exact

TsdfCloud = namedtuple("TsdfCloud", ["xyz", "edge"])
FusedFrame = namedtuple("FusedFrame", ["transformation", "fitness", "inlier_rmse", "status", "integrated"])
FusedPrediction = namedtuple("FusedPrediction", ["confidences", "xyz", "edge"])


# ------------------------------------------------------------------------------------------------------------- the contract
def world_to_camera(pose: np.ndarray) -> np.ndarray:
    """The twelve float32 of the contract from a checked camera-to-world pose (4, 4) float64: R^T row-major, then -(R^T t)."""
    Rt = pose[:3, :3].T
    return np.concatenate((Rt.reshape(-1), -(Rt @ pose[:3, 3]))).astype(_F32)


def centres_host(o, voxel, n: int) -> np.ndarray:
    """(n,) float32: o + (float32(i) + 0.5) * voxel for i = 0 .. n-1."""
    return _F32(o) + (np.arange(n).astype(_F32) + _F32(0.5)) * _F32(voxel)


def integrate_host(tsdf, weight, origin, voxel, trunc, max_weight, depth, camera, z_lo, z_hi, w2c) -> None:
    """One frame into tsdf and weight (nz, ny, nx) float32, in place, by the contract: one layer of voxels at a time."""
    nz, ny, nx = tsdf.shape
    H, W = depth.shape
    r, t = w2c[:9].reshape(3, 3), w2c[9:]
    cx, cy, cz = (centres_host(o, voxel, n) for o, n in zip(origin, (nx, ny, nz)))
    cx, cy = cx[None, :], cy[:, None]
    one, half, mw, trunc = _F32(1), _F32(0.5), _F32(max_weight), _F32(trunc)
    Wf, Hf = _F32(W), _F32(H)
    flat = depth.reshape(-1)
    with np.errstate(all="ignore"):
        plane = [r[a, 0] * cx + r[a, 1] * cy for a in range(3)]           # (the first sum does not depend on the layer)
        for k in range(nz):
            qx, qy, qz = ((plane[a] + r[a, 2] * cz[k]) + t[a] for a in range(3))
            ok = qz > 0
            uf = ((qx / qz) * camera.fx + camera.ppx) + half
            vf = ((qy / qz) * camera.fy + camera.ppy) + half
            ok &= (uf >= 0) & (uf < Wf) & (vf >= 0) & (vf < Hf)
            if not ok.any():
                continue
            u = np.where(ok, uf, 0).astype(np.int64)
            v = np.where(ok, vf, 0).astype(np.int64)
            d = flat[v * W + u]
            ok &= d != 0
            z = d.astype(_F32) * camera.depth_scale
            ok &= (z_lo < z) & (z < z_hi)
            sdf = z - qz
            ok &= ~(sdf < -trunc)
            s = sdf / trunc
            s = np.where(s > one, one, s)
            w = weight[k]
            w1 = w + one
            tsdf[k] = np.where(ok, (tsdf[k] * w + s) / w1, tsdf[k])
            weight[k] = np.where(ok, np.where(w1 > mw, mw, w1), w)


def extract_host(tsdf, weight, origin, voxel, min_weight) -> TsdfCloud:
    """The surface points of tsdf and weight (nz, ny, nx) float32 by the contract."""
    nz, ny, nx = tsdf.shape
    heavy, neg = weight >= _F32(min_weight), tsdf < 0
    emit = np.zeros((nz, ny, nx, 3), bool)
    emit[:, :, :-1, 0] = heavy[:, :, :-1] & heavy[:, :, 1:] & (neg[:, :, :-1] != neg[:, :, 1:])
    emit[:, :-1, :, 1] = heavy[:, :-1] & heavy[:, 1:] & (neg[:, :-1] != neg[:, 1:])
    emit[:-1, :, :, 2] = heavy[:-1] & heavy[1:] & (neg[:-1] != neg[1:])
    edge = np.flatnonzero(emit.reshape(-1)).astype(np.int64)
    n = edge // 3
    a = edge - 3 * n
    row = n // nx
    ijk = np.stack((n - row * nx, row % ny, row // ny), axis=1)
    t = tsdf.reshape(-1)
    tn, tb = t[n], t[n + np.array([1, nx, nx * ny], np.int64)[a]]
    with np.errstate(all="ignore"):
        f = tn / (tn - tb)
        xyz = np.stack([centres_host(origin[c], voxel, dim)[ijk[:, c]] for c, dim in enumerate((nx, ny, nz))], axis=1)
        rows = np.arange(edge.shape[0])
        xyz[rows, a] = xyz[rows, a] + f * _F32(voxel)
    return TsdfCloud(np.ascontiguousarray(xyz.astype(_F32, copy=False).reshape(-1, 3)), edge)


# --------------------------------------------------------------------------------------------------------------- the volume
def _check_camera(camera, who: str) -> None:
    if not isinstance(camera, D.DepthCamera):
        raise ValueError(f"{who}: camera={camera!r} must be a DepthCamera")
    if camera.coeffs is not None:
        raise ValueError(f"{who}: a camera with coeffs is not taken: the inverse Brown-Conrady model is closed form only in "
                         "the deprojecting direction")
    if camera.width >= MAX_SIDE or camera.height >= MAX_SIDE:
        raise ValueError(f"{who}: a frame of {camera.height} x {camera.width} pixels: width and height must be below 2^24")


class TsdfVolume:
    """The dense volume of the module docstring and its state: tsdf and weight (nz, ny, nx) float32 - numpy arrays when the
    volume lies on the host, device tensors when it lies on a cuda device (csrc/tsdf.hip), the same bits either way."""

    def __init__(self, origin, voxel, dims, trunc=None, max_weight: int = 64, device=None):
        import torch
        who = "TsdfVolume"
        if isinstance(origin, (str, bytes)) or np.shape(origin) != (3,):
            raise ValueError(f"{who}: origin={origin!r} must be three numbers (ox, oy, oz)")
        self.origin = tuple(D._scalar(o, f"origin[{a}]", who, False) for a, o in enumerate(origin))
        self.voxel = D._scalar(voxel, "voxel", who, True)
        if isinstance(dims, (str, bytes)) or np.shape(dims) != (3,):
            raise ValueError(f"{who}: dims={dims!r} must be three integers (nx, ny, nz)")
        self.dims = tuple(D._integer(n, f"dims[{a}]", who, 1) for a, n in enumerate(dims))
        nx, ny, nz = self.dims
        if nx * ny * nz >= MAX_VOXELS:
            raise ValueError(f"{who}: dims={self.dims} are {nx * ny * nz} voxels, outside 1 .. 2^31 - 1")
        with np.errstate(over="ignore"):
            self.trunc = D._scalar(_F32(4) * self.voxel if trunc is None else trunc, "trunc", who, True)
        self.max_weight = D._integer(max_weight, "max_weight", who, MIN_WEIGHT, MAX_WEIGHT)
        self.device = torch.device(("cuda" if torch.cuda.is_available() else "cpu") if device is None else device)
        self.reset()

    @property
    def shape(self):
        nx, ny, nz = self.dims
        return (nz, ny, nx)

    @property
    def on_device(self) -> bool:
        return self.device.type == "cuda"

    def reset(self) -> None:
        """All 1.0 and all 0.0, as at the start."""
        if self.on_device:
            import torch
            self.tsdf = torch.ones(self.shape, dtype=torch.float32, device=self.device)
            self.weight = torch.zeros(self.shape, dtype=torch.float32, device=self.device)
        else:
            self.tsdf, self.weight = np.ones(self.shape, _F32), np.zeros(self.shape, _F32)

    def to(self, device) -> "TsdfVolume":
        """This volume with its state moved to `device` (itself when it lies there already)."""
        import torch
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", self.device.index if self.on_device else torch.cuda.current_device())
        if device == self.device or (device.type == "cpu" and not self.on_device):
            return self
        host = not self.on_device
        if device.type == "cuda":
            self.tsdf, self.weight = (torch.from_numpy(x).to(device) if host else x.to(device) for x in (self.tsdf, self.weight))
        else:
            self.tsdf, self.weight = self.tsdf.cpu().numpy(), self.weight.cpu().numpy()
        self.device = device
        return self

    def integrate(self, depth, camera, pose=None, z_range=(0.05, 0.6)) -> None:
        """One depth frame (H, W) uint16 seen from `pose`, the (4, 4) camera-to-world transform, into the volume: one
        rl_tsdf_integrate launch on a cuda volume (a numpy frame is uploaded, 2 bytes per pixel), integrate_host otherwise."""
        who = "TsdfVolume.integrate"
        _check_camera(camera, who)
        z_lo, z_hi, _ = D.check_inputs(depth, camera, z_range, 1, who)
        w2c = world_to_camera(np.eye(4) if pose is None else R.check_transform(pose, f"{who}: pose"))
        if not self.on_device:
            integrate_host(self.tsdf, self.weight, self.origin, self.voxel, self.trunc, self.max_weight, D._host(depth), camera,
                           z_lo, z_hi, w2c)
            return
        import torch
        from .. import _ops as ops
        with torch.cuda.device(self.device), torch.no_grad():
            ops.tsdf_integrate(self.tsdf, self.weight, self.origin, self.voxel, self.trunc, self.max_weight,
                               D._upload(depth, self.device), camera, z_lo, z_hi, w2c)

    def extract(self, min_weight: int = 1) -> TsdfCloud:
        """The surface as points: TsdfCloud(xyz (M, 3) float32, edge (M,) int64), ascending in edge - device tensors from a
        cuda volume (rl_tsdf_count, one read-back of M, rl_tsdf_points), numpy arrays otherwise."""
        min_weight = D._integer(min_weight, "min_weight", "TsdfVolume.extract", MIN_WEIGHT, self.max_weight)
        if not self.on_device:
            return extract_host(self.tsdf, self.weight, self.origin, self.voxel, min_weight)
        import torch
        from .. import _ops as ops
        with torch.cuda.device(self.device), torch.no_grad():
            return TsdfCloud(*ops.tsdf_extract(self.tsdf, self.weight, self.origin, self.voxel, min_weight))


# ---------------------------------------------------------------------------------------------------------- the camera loop
class DepthFusion:
    """The loop of a camera that keeps delivering frames, around a model: add(depth) registers the frame against the surface
    of `volume` (frame to model) and integrates it there, predict() votes on that surface.

    model: a Model; the volume is placed on model.device, and a model placed on the CPU runs the numpy twins with the same
    bits.  camera: a DepthCamera without coeffs.  icp: an IcpSettings - frames after the first are tracked - or None - every
    frame after the first needs its pose.  temporal: a TemporalFilter or None; with one, tracking and integration both see the
    filtered frame.  z_range: the pixels that take part.  track_stride: every track_stride-th row and column makes the source
    cloud of the registration (the integration always reads the whole frame).  min_weight: of the surface the frames are
    registered against and predict() votes on."""

    def __init__(self, model, camera, volume, *, icp=None, temporal=None, z_range=(0.05, 0.6), track_stride: int = 1,
                 min_weight: int = 1):
        who = "DepthFusion"
        if not hasattr(model, "predict_scene") or not hasattr(model, "device"):
            raise ValueError(f"{who}: model={model!r} must be a Model")
        _check_camera(camera, who)
        if not isinstance(volume, TsdfVolume):
            raise ValueError(f"{who}: volume={volume!r} must be a TsdfVolume")
        if icp is not None and not isinstance(icp, R.IcpSettings):
            raise ValueError(f"{who}: icp={icp!r} must be an IcpSettings or None")
        if temporal is not None and not isinstance(temporal, D.TemporalFilter):
            raise ValueError(f"{who}: temporal={temporal!r} must be a TemporalFilter or None")
        D.check_inputs(np.zeros((1, 1), np.uint16), D.DepthCamera(1, 1, 1.0, 1.0, 0.0, 0.0, 1.0), z_range, track_stride, who)
        self.min_weight = D._integer(min_weight, "min_weight", who, MIN_WEIGHT, volume.max_weight)
        self.model, self.camera, self.icp, self.temporal = model, camera, icp, temporal
        self.z_range, self.track_stride = z_range, track_stride
        self.volume = volume.to(model.device)
        self._poses = []

    @property
    def transformations(self) -> np.ndarray:
        """(frames, 4, 4) float64: the camera-to-world poses so far."""
        return np.array(self._poses, np.float64).reshape(-1, 4, 4)

    def reset(self) -> None:
        """Clears the volume, the temporal filter and the poses."""
        self.volume.reset()
        if self.temporal is not None:
            self.temporal.reset()
        self._poses = []

    def add(self, depth, pose=None) -> FusedFrame:
        """One more frame (H, W) uint16.  Frame 0 is integrated at `pose` (None: the identity), status "reference", fitness
        1, rmse 0.  A later frame starts from init = pose if given, else the previous frame's transformation.  Without icp
        the pose is required and the frame is integrated there, status "given" (fitness 1 and rmse 0: nothing was measured).
        With icp the frame's points - depth_points(frame, camera, None, z_range, track_stride) - are registered onto
        volume.extract(min_weight).xyz by registration.icp(source, target, init=init, **asdict(icp)) - icp_device on a GPU
        model, everything staying in HBM - and the frame is integrated at the result; status "degenerate": the frame is not
        integrated and the stored transformation stays init.  A frame without a pixel inside z_range raises ValueError; a
        surface with too few points for the ICP's normals is ICP's own refusal.  Returns FusedFrame(transformation (4, 4)
        float64, fitness, inlier_rmse, status, integrated)."""
        who = "DepthFusion.add"
        device = self.model.device
        on_gpu = device.type == "cuda"
        D.check_inputs(depth, self.camera, self.z_range, self.track_stride, who)
        if self.temporal is not None:
            self.temporal._check(depth, who)
        given = None if pose is None else R.check_transform(pose, f"{who}: pose")
        first = not self._poses
        if not first and self.icp is None and given is None:
            raise ValueError(f"{who}: without icp every frame after the first needs its pose")
        frame = depth if self.temporal is None else self.temporal.process(depth, device)
        cloud = D.depth_points(frame, self.camera, None, self.z_range, self.track_stride, device)
        if cloud.xyz.shape[0] == 0:
            raise ValueError(f"{who}: no pixel inside z_range")
        fitness, rmse, integrated = 1.0, 0.0, True
        if first:
            T, status = (np.eye(4) if given is None else given), "reference"
        elif self.icp is None:
            T, status = given, "given"
        else:
            init = given if given is not None else self._poses[-1]
            target = self.volume.extract(self.min_weight).xyz
            settings = asdict(self.icp)
            max_distance = settings.pop("max_distance")
            if on_gpu:
                chk = R.check_parameters(max_distance, init=init, who=who, **settings)
                res = R.icp_device(cloud.xyz, target, None, chk, device, who)
            else:
                res = R.icp_host(cloud.xyz, target, max_distance=max_distance, init=init, **settings)
            T, fitness, rmse, status = res.transformation, float(res.fitness), float(res.inlier_rmse), res.status
            if status == "degenerate":
                T, integrated = init, False
        T = np.array(T, np.float64)
        if integrated:
            self.volume.integrate(frame, self.camera, T, self.z_range)
        self._poses.append(T)
        return FusedFrame(T.copy(), fitness, rmse, status, integrated)

    def surface(self) -> TsdfCloud:
        """volume.extract(min_weight): device tensors on a GPU model."""
        return self.volume.extract(self.min_weight)

    def predict(self, **predict_scene_keywords) -> FusedPrediction:
        """model.predict_scene(surface().xyz, None, **keywords) - on the GPU the device tensor goes in as it is -:
        FusedPrediction(confidences (C, M) float32, xyz (M, 3) float32, edge (M,) int64) as numpy arrays.  The return_*
        keywords are not taken; an empty surface raises ValueError."""
        for name in ("return_counts", "return_outliers", "return_planes"):
            if predict_scene_keywords.get(name):
                raise ValueError(f"DepthFusion.predict: {name} is not taken; call predict_scene on surface().xyz for it")
        surf = self.surface()
        if surf.xyz.shape[0] == 0:
            raise ValueError("DepthFusion.predict: the surface is empty")
        conf = self.model.predict_scene(surf.xyz, None, **predict_scene_keywords)
        xyz, edge = (x.cpu().numpy() if D._is_tensor(x) else x for x in surf)
        return FusedPrediction(conf, xyz, edge)
