"""Depth frames to points: the stage between a depth camera's raw z16 frame and the (M, 3) cloud every other entry starts
from - what the reference's camera loop does on the host (camera/realsense_camera.py:90-125: a temporal filter over the frame,
rs.pointcloud().calculate, then points[(0.05 < z) & (z < 0.6)]).  The camera driver stays out of scope; this is the arithmetic
after it.

This module is the numpy host twin of csrc/depth.hip (include/rl_randlanet.h, rl_depth_*) and the public deproject /
TemporalFilter / depth_points.  The twin's arithmetic is the specification; the kernels equal it bit for bit.  All arithmetic is
float32, one correctly rounded operation at a time, in the order written here:

  camera         DepthCamera(width, height, fx, fy, ppx, ppy, depth_scale, coeffs=None), immutable, the scalars stored as
                 float32.  coeffs: None (pinhole) or (k1, k2, p1, p2, k3) of the INVERSE Brown-Conrady model, which is closed
                 form: no iteration
  depth          (H, W) uint16, C-contiguous - a numpy array, or a torch tensor on the device
  takes part     pixel (v, u) when v % stride == 0 and u % stride == 0
  point          with the raw value d: z = float32(d) * depth_scale; x0 = (float32(u) - ppx) / fx, y0 = (float32(v) - ppy) / fy;
                 with coeffs r2 = x0*x0 + y0*y0, f = 1 + r2*(k1 + r2*(k2 + r2*k3)) (innermost first),
                 xd = x0*f + ((2*p1)*(x0*y0) + p2*(r2 + 2*(x0*x0))), yd = y0*f + ((2*p2)*(x0*y0) + p1*(r2 + 2*(y0*y0))), and
                 xd, yd replace x0, y0; the point is (x0*z, y0*z, z)
  kept           when d != 0 and z_lo < z and z < z_hi: both comparisons strict and in float32, z_lo and z_hi rounded to
                 float32 once
  outputs        DepthCloud(xyz (M, 3) float32, pixel (M,) int32 = v * W + u): the kept points in row-major pixel order, what
                 points[filter] gives the reference.  M = 0 is a valid result with empty arrays.  numpy arrays on the host
                 path, device tensors on the device path
  temporal       TemporalFilter(alpha=0.33, delta=100): librealsense's temporal filter with persistence off, restated here as
                 this project's own contract.  The state is a uint16 image, all 0 at the start.  Per pixel with current value c
                 and state p: c == 0 -> output 0, state unchanged; p == 0 -> output c, state c; abs(int(c) - int(p)) < delta ->
                 f = (alpha*float32(c) + one_minus_alpha*float32(p)) + 0.5, output min(65535, trunc(f)), state that output;
                 otherwise output c, state c.  one_minus_alpha = float32(1) - float32(alpha) is made once, on the host
  refusals       all ValueError, before any work: a depth of the wrong dtype, ndim or shape against the camera, or not
                 C-contiguous; stride < 1; fx, fy or depth_scale not finite and greater than 0; z_lo >= z_hi; alpha outside
                 (0, 1]; delta outside 1 .. 65535; H*W >= 2^31; a frame of another shape than the filter's state

Not here: batches of frames, intensity or colour as features, the alignment of a colour image, librealsense's persistence
modes, spatial filter and hole filling.
"""
from collections import namedtuple

import numpy as np

_F32 = np.float32
MAX_PIXELS = 2 ** 31
MIN_DELTA, MAX_DELTA = 1, 65535

DepthCloud = namedtuple("DepthCloud", ["xyz", "pixel"])
_Camera = namedtuple("DepthCamera", ["width", "height", "fx", "fy", "ppx", "ppy", "depth_scale", "coeffs"])


def _integer(value, name: str, who: str, low: int, high=None) -> int:
    try:
        ok = not isinstance(value, (bool, str, bytes)) and int(value) == value and int(value) >= low
        ok = ok and (high is None or int(value) <= high)
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        bound = f">= {low}" if high is None else f"in {low} .. {high}"
        raise ValueError(f"{who}: {name}={value!r} must be an integer {bound}")
    return int(value)


def _scalar(value, name: str, who: str, positive: bool):
    try:
        with np.errstate(over="ignore"):
            x = _F32(value)
    except (TypeError, ValueError):
        x = _F32(np.nan)
    if isinstance(value, (bool, str, bytes)) or not np.isfinite(x) or (positive and not x > 0):
        raise ValueError(f"{who}: {name}={value!r} must be finite" + (" and greater than 0" if positive else ""))
    return x


class DepthCamera(_Camera):
    """The intrinsics of a depth stream: width, height (pixels), fx, fy (focal lengths in pixels), ppx, ppy (the principal
    point), depth_scale (metres per raw unit) and coeffs - None for a pinhole, or (k1, k2, p1, p2, k3) of the inverse
    Brown-Conrady model.  Immutable; the scalars are float32.  See the module docstring."""
    __slots__ = ()

    def __new__(cls, width, height, fx, fy, ppx, ppy, depth_scale, coeffs=None):
        who = "DepthCamera"
        width, height = _integer(width, "width", who, 1), _integer(height, "height", who, 1)
        if width * height >= MAX_PIXELS:
            raise ValueError(f"{who}: width={width} x height={height} is {width * height} pixels, outside 1 .. 2^31 - 1")
        fx, fy = _scalar(fx, "fx", who, True), _scalar(fy, "fy", who, True)
        ppx, ppy = _scalar(ppx, "ppx", who, False), _scalar(ppy, "ppy", who, False)
        depth_scale = _scalar(depth_scale, "depth_scale", who, True)
        if coeffs is not None:
            if isinstance(coeffs, (str, bytes)) or np.shape(coeffs) != (5,):
                raise ValueError(f"{who}: coeffs={coeffs!r} must be None or five numbers (k1, k2, p1, p2, k3)")
            coeffs = tuple(_scalar(c, f"coeffs[{j}]", who, False) for j, c in enumerate(coeffs))
        return super().__new__(cls, width, height, fx, fy, ppx, ppy, depth_scale, coeffs)


def _is_tensor(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr")


def check_inputs(depth, camera, z_range=(0.05, 0.6), stride=1, who="deproject"):
    """The refusals of deproject, all ValueError, before any work.  depth: a numpy array or a torch tensor.  Returns z_lo and
    z_hi as float32 and stride as int."""
    if not isinstance(camera, DepthCamera):
        raise ValueError(f"{who}: camera={camera!r} must be a DepthCamera")
    stride = _integer(stride, "stride", who, 1)
    if isinstance(z_range, (str, bytes)) or np.shape(z_range) != (2,):
        raise ValueError(f"{who}: z_range={z_range!r} must be a pair (z_lo, z_hi)")
    try:
        with np.errstate(over="ignore"):
            z_lo, z_hi = _F32(z_range[0]), _F32(z_range[1])
    except (TypeError, ValueError):
        raise ValueError(f"{who}: z_range={z_range!r} must be a pair of numbers") from None
    if not z_lo < z_hi:
        raise ValueError(f"{who}: z_range={z_range!r}: z_lo must be below z_hi")
    check_frame(depth, (camera.height, camera.width), who)
    return z_lo, z_hi, stride


def check_frame(depth, shape=None, who="deproject") -> None:
    """A frame is a uint16 (H, W) numpy array or torch tensor, C-contiguous, of fewer than 2^31 pixels - and of `shape`."""
    tensor = _is_tensor(depth)
    if not tensor and not isinstance(depth, np.ndarray):
        raise ValueError(f"{who}: depth must be a numpy array or a torch tensor, not {type(depth).__name__}")
    dtype = str(depth.dtype).replace("torch.", "")
    if dtype != "uint16":
        raise ValueError(f"{who}: depth has dtype {dtype}, expected uint16")
    got = tuple(int(s) for s in depth.shape)
    if len(got) != 2:
        raise ValueError(f"{who}: depth has shape {got}, expected (H, W)")
    if shape is not None and got != tuple(shape):
        raise ValueError(f"{who}: depth has shape {got}, expected {tuple(shape)}")
    if got[0] < 1 or got[1] < 1 or got[0] * got[1] >= MAX_PIXELS:
        raise ValueError(f"{who}: depth has {got[0]} x {got[1]} pixels, outside 1 .. 2^31 - 1")
    if not (depth.is_contiguous() if tensor else depth.flags.c_contiguous):
        raise ValueError(f"{who}: depth must be C-contiguous")


def _host(depth) -> np.ndarray:
    return depth.cpu().numpy() if _is_tensor(depth) else depth


def _device_of(depth, device):
    """The device a call runs on: `device`; without one the tensor's own, else cuda when there is one."""
    import torch
    if device is None:
        if _is_tensor(depth):
            return depth.device
        return torch.device("cuda" if torch.cuda.is_available() else "cpu")
    return torch.device(device)


def _upload(depth, device):
    import torch
    if _is_tensor(depth):
        return depth if depth.device == device else depth.to(device)
    return torch.from_numpy(depth).to(device)


def rays_host(u: np.ndarray, v: np.ndarray, camera: DepthCamera):
    """(x0, y0) float32 of the pixels (v, u) - integer arrays - by the contract: pinhole, then the inverse Brown-Conrady model
    when the camera has coefficients."""
    x = (u.astype(_F32) - camera.ppx) / camera.fx
    y = (v.astype(_F32) - camera.ppy) / camera.fy
    if camera.coeffs is not None:
        k1, k2, p1, p2, k3 = camera.coeffs
        two = _F32(2)
        r2 = x * x + y * y
        f = _F32(1) + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = x * f + ((two * p1) * (x * y) + p2 * (r2 + two * (x * x)))
        yd = y * f + ((two * p2) * (x * y) + p1 * (r2 + two * (y * y)))
        x, y = xd, yd
    return x, y


def deproject_host(depth, camera: DepthCamera, z_range=(0.05, 0.6), stride: int = 1) -> DepthCloud:
    """The numpy twin of the device deprojection; see the module docstring for the contract."""
    z_lo, z_hi, stride = check_inputs(depth, camera, z_range, stride)
    d = _host(depth)
    H, W = d.shape
    z = d.astype(_F32) * camera.depth_scale
    keep = (d != 0) & (z_lo < z) & (z < z_hi)
    if stride > 1:
        part = np.zeros((H, W), bool)
        part[::stride, ::stride] = True
        keep &= part
    pixel = np.flatnonzero(keep)
    v = pixel // W
    u = pixel - v * W
    x, y = rays_host(u, v, camera)
    zk = z.reshape(-1)[pixel]
    xyz = np.stack((x * zk, y * zk, zk), axis=1).astype(_F32, copy=False).reshape(-1, 3)
    return DepthCloud(np.ascontiguousarray(xyz), pixel.astype(np.int32))


def temporal_host(depth: np.ndarray, state: np.ndarray, alpha, one_minus_alpha, delta: int):
    """One frame of the temporal filter by the contract: (output, new state), both (H, W) uint16; alpha and one_minus_alpha
    float32."""
    c, p = depth.astype(np.int32), state.astype(np.int32)
    blend = (p != 0) & (np.abs(c - p) < delta)
    f = (_F32(alpha) * c.astype(_F32) + _F32(one_minus_alpha) * p.astype(_F32)) + _F32(0.5)
    out = np.where(blend, np.minimum(f.astype(np.int32), 65535), c)       # (astype truncates; f >= 0.5)
    out = np.where(c == 0, 0, out)
    new = np.where(c == 0, p, out)
    return out.astype(np.uint16), new.astype(np.uint16)


class TemporalFilter:
    """The temporal filter of the module docstring and its state - a numpy array on the host path, a device tensor on the
    device path, all 0 at the start and after reset().  process(depth) returns the filtered frame and updates the state; a
    frame of another shape than the state's raises ValueError."""

    def __init__(self, alpha: float = 0.33, delta: int = 100):
        try:
            a = _F32(alpha)
        except (TypeError, ValueError):
            a = _F32(np.nan)
        if isinstance(alpha, (bool, str, bytes)) or not (a > 0 and a <= 1):
            raise ValueError(f"TemporalFilter: alpha={alpha!r} must lie in (0, 1]")
        self.alpha = a
        self.one_minus_alpha = _F32(1) - a
        self.delta = _integer(delta, "delta", "TemporalFilter", MIN_DELTA, MAX_DELTA)
        self._state = None

    def reset(self) -> None:
        self._state = None

    @property
    def state(self):
        """The state: None before the first frame (all 0, of any shape), else a numpy array or a device tensor."""
        return self._state

    def _check(self, depth, who: str) -> None:
        check_frame(depth, None, who)
        if self._state is not None and tuple(self._state.shape) != tuple(depth.shape):
            raise ValueError(f"{who}: depth has shape {tuple(depth.shape)}, the filter's state {tuple(self._state.shape)} "
                             "(reset() starts over)")

    def _host_state(self, shape) -> np.ndarray:
        if self._state is None:
            self._state = np.zeros(shape, np.uint16)
        elif _is_tensor(self._state):
            self._state = self._state.cpu().numpy()
        return self._state

    def _device_state(self, shape, device):
        import torch
        if self._state is None:
            self._state = torch.zeros(shape, dtype=torch.int16, device=device).view(torch.uint16)
        elif not _is_tensor(self._state):
            self._state = torch.from_numpy(self._state).to(device)
        elif self._state.device != device:
            self._state = self._state.to(device)
        return self._state

    def process(self, depth, device=None):
        """The filtered frame of `depth` (H, W) uint16: a numpy array from the host path, a device tensor from the device
        path (csrc/depth.hip, one launch, the state resident), the same bits."""
        import torch
        self._check(depth, "TemporalFilter.process")
        device = _device_of(depth, device)
        if device.type != "cuda":
            out, self._state = temporal_host(_host(depth), self._host_state(tuple(depth.shape)), self.alpha,
                                             self.one_minus_alpha, self.delta)
            return out
        from .. import _ops as ops
        with torch.cuda.device(device), torch.no_grad():
            state = self._device_state(tuple(depth.shape), device)
            return ops.temporal_filter(_upload(depth, device), state, self.alpha, self.one_minus_alpha, self.delta)


def deproject(depth, camera: DepthCamera, z_range=(0.05, 0.6), stride: int = 1, device=None) -> DepthCloud:
    """The cloud of one depth frame: DepthCloud(xyz (M, 3) float32, pixel (M,) int32) - see the module docstring.  Runs on
    the GPU (csrc/depth.hip) when `device` is a cuda device, or when it is None and depth is a device tensor or a GPU is
    available - the result is then device tensors, ready for Model.predict_scene / predict_keypoints -; otherwise
    deproject_host and numpy arrays.  The same bits either way."""
    return depth_points(depth, camera, None, z_range, stride, device)


def depth_points(depth, camera: DepthCamera, temporal: TemporalFilter = None, z_range=(0.05, 0.6), stride: int = 1,
                 device=None) -> DepthCloud:
    """temporal.process(depth), when a filter is given, then deproject of its output - on the device one fused entry
    (rl_depth_points: three launches, the state updated in the last one) and one read-back, of M."""
    import torch
    z_lo, z_hi, stride = check_inputs(depth, camera, z_range, stride, "depth_points")
    if temporal is not None:
        if not isinstance(temporal, TemporalFilter):
            raise ValueError(f"depth_points: temporal={temporal!r} must be a TemporalFilter or None")
        temporal._check(depth, "depth_points")
    device = _device_of(depth, device)
    if device.type != "cuda":
        frame = _host(depth) if temporal is None else temporal.process(depth, device)
        return deproject_host(frame, camera, (z_lo, z_hi), stride)
    from .. import _ops as ops
    with torch.cuda.device(device), torch.no_grad():
        state = None if temporal is None else temporal._device_state(tuple(depth.shape), device)
        filt = None if temporal is None else (temporal.alpha, temporal.one_minus_alpha, temporal.delta)
        xyz, pixel, _ = ops.depth_points(_upload(depth, device), camera, z_lo, z_hi, stride, state, filt)
        return DepthCloud(xyz, pixel)


class DepthPrediction(namedtuple("DepthPrediction", ["confidences", "xyz", "pixel"])):
    """Model.predict_depth's result: confidences (C, M) float32, xyz (M, 3) float32 and pixel (M,) int32 of the kept points."""
    __slots__ = ()

    def image(self, height: int, width: int, fill: float = 0.0) -> np.ndarray:
        """The confidences scattered back to the pixels: (C, height, width) float32, column j at pixel[j], `fill` elsewhere."""
        height, width = _integer(height, "height", "DepthPrediction.image", 1), _integer(width, "width", "DepthPrediction.image", 1)
        if self.pixel.size and (int(self.pixel.min()) < 0 or int(self.pixel.max()) >= height * width):
            raise ValueError(f"DepthPrediction.image: pixel indices outside a {height} x {width} frame")
        out = np.full((self.confidences.shape[0], height * width), fill, np.float32)
        out[:, self.pixel] = self.confidences
        return out.reshape(-1, height, width)
