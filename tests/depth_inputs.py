"""Shared inputs and yardsticks of the depth tests (test_depth_*): the cameras, the seeded synthetic frames, the temporal
sequence, scalar yardsticks that are independent of the package's vectorised twin (np.float32 scalars, one operation per
statement, in the order of utils/depth.py's docstring), and the twin's result per case (computed once, never modified).  A case
is (depth (H, W) uint16, camera, z_range, stride)."""
import numpy as np

F32 = np.float32
SCALE = 0.00025
Z_RANGE = (0.05, 0.6)                    # raw values 201 .. 2399 are inside
COEFFS = (0.11, -0.23, 0.0013, -0.0021, 0.07)
ALPHA, DELTA = 0.33, 100
_cases, _twins = {}, {}

# H x W of the device tests: one pixel; below one chunk of 1024 and no multiple of 8 or 64; exactly one chunk, and one pixel
# more; more than 256 chunks (the scan's per-thread run exceeds one); the reference's frame
SHAPES = ((1, 1), (3, 67), (1, 1024), (1, 1025), (257, 1031))
CONTENTS = ("zero", "all", "last", "first", "random")
CASES = tuple(f"{h}x{w}-{c}" for h, w in SHAPES for c in CONTENTS) + (
    "3x67-random-coeffs", "257x1031-random-coeffs",
    "3x67-random-stride2", "3x67-random-stride3", "257x1031-random-stride2", "257x1031-random-stride3",
    "3x67-all-stride2", "5x67-random", "5x67-random-coeffs", "5x67-random-stride2", "5x67-random-stride3",
    "768x1024-random")
SCALAR = ("5x67-random", "5x67-random-coeffs", "5x67-random-stride2", "5x67-random-stride3", "3x67-random-stride3",
          "1x1-all", "1x1-zero", "3x67-first", "3x67-last")       # the cases small enough for the scalar yardstick


def camera(H, W, coeffs=False):
    """Intrinsics that are deliberately not round, so every rounding matters."""
    from randlanet.utils.depth import DepthCamera
    return DepthCamera(W, H, 730.5, 731.25, W / 2 - 0.2, H / 2 + 0.3, SCALE, COEFFS if coeffs else None)


def contents(H, W, kind, seed):
    rs = np.random.RandomState(seed)
    d = np.zeros((H, W), np.uint16)
    if kind == "all":
        d[:] = rs.randint(400, 2000, (H, W))
    elif kind == "last":
        d[-1, -1] = 1000
    elif kind == "first":
        d[0, 0] = 1000
    elif kind == "random":           # about half inside z_range, a tenth holes: the lanes' masks differ
        d[:] = rs.randint(1, 4800, (H, W))
        d[rs.uniform(size=(H, W)) < 0.1] = 0
    elif kind != "zero":
        raise KeyError(kind)
    return d


def case(name):
    if name not in _cases:
        parts = name.split("-")
        H, W = (int(s) for s in parts[0].split("x"))
        d = contents(H, W, parts[1], sum(map(ord, parts[0] + parts[1])))      # (the variants of a frame share its content)
        stride = int(parts[2][6:]) if len(parts) > 2 and parts[2].startswith("stride") else 1
        d.setflags(write=False)
        _cases[name] = (d, camera(H, W, "coeffs" in parts), Z_RANGE, stride)
    return _cases[name]


def _frozen(cloud):
    for a in cloud:
        a.setflags(write=False)
    return cloud


def twin(name):
    if name not in _twins:
        from randlanet.utils.depth import deproject_host
        _twins[name] = _frozen(deproject_host(*case(name)))
    return _twins[name]


def assert_same(got, want, what=""):
    """Two DepthClouds (numpy arrays or tensors), bit for bit."""
    gx, gp = (np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a) for a in got)
    assert gx.dtype == np.float32 and gp.dtype == np.int32, what
    assert gx.shape == want.xyz.shape and gp.shape == want.pixel.shape, (what, gx.shape, want.xyz.shape)
    assert np.array_equal(gp, want.pixel), what
    assert np.array_equal(gx.view(np.uint32), want.xyz.view(np.uint32)), what


def yardstick(depth, cam, z_range, stride):
    """(xyz, pixel) by an independent scalar loop: np.float32 scalars, one operation per statement."""
    H, W = depth.shape
    z_lo, z_hi = F32(z_range[0]), F32(z_range[1])
    fx, fy, ppx, ppy, scale = F32(cam.fx), F32(cam.fy), F32(cam.ppx), F32(cam.ppy), F32(cam.depth_scale)
    xyz, pixel = [], []
    for v in range(H):
        for u in range(W):
            if v % stride != 0 or u % stride != 0:
                continue
            d = int(depth[v, u])
            z = F32(d) * scale
            if not (d != 0 and z_lo < z and z < z_hi):
                continue
            x = F32(u) - ppx
            x = x / fx
            y = F32(v) - ppy
            y = y / fy
            if cam.coeffs is not None:
                k1, k2, p1, p2, k3 = (F32(c) for c in cam.coeffs)
                xx = x * x
                yy = y * y
                r2 = xx + yy
                f = r2 * k3
                f = k2 + f
                f = r2 * f
                f = k1 + f
                f = r2 * f
                f = F32(1) + f
                xy = x * y
                a = F32(2) * p1
                a = a * xy
                b = F32(2) * xx
                b = r2 + b
                b = p2 * b
                t = a + b
                xd = x * f
                xd = xd + t
                a = F32(2) * p2
                a = a * xy
                b = F32(2) * yy
                b = r2 + b
                b = p1 * b
                t = a + b
                yd = y * f
                yd = yd + t
                x, y = xd, yd
            xyz.append((x * z, y * z, z))
            pixel.append(v * W + u)
    return np.array(xyz, F32).reshape(-1, 3), np.array(pixel, np.int32)


# ---------------------------------------------------------------------------------------------------- the temporal sequence
T_SHAPE = (3, 67)
# pixel (flat index): what it is there for
T_FIRST, T_HOLE, T_BELOW, T_AT, T_HALF, T_TOP, T_NEVER = 0, 1, 2, 3, 4, 5, 6


def temporal_frames():
    """Five (3, 67) frames whose pixels between them take every branch of the filter: the designed pixels 0 .. 6, the others a
    random walk of steps up to +-150 around the previous frame with a tenth of holes."""
    rs = np.random.RandomState(31)
    n = T_SHAPE[0] * T_SHAPE[1]
    frames = [rs.randint(300, 3000, n)]
    for _ in range(4):
        frames.append(np.clip(frames[-1] + rs.randint(-150, 151, n), 1, 65535))
    frames = [np.where(rs.uniform(size=n) < 0.1, 0, f) for f in frames]
    designed = {T_FIRST: (1000, 1000, 1000, 1000, 1000),
                T_HOLE: (1000, 0, 1040, 0, 0),               # a hole keeps the state; the frame after it blends with 1000
                T_BELOW: (1000, 1099, 1000, 1000, 1000),     # a difference of delta - 1: blended
                T_AT: (1000, 1100, 1000, 1100, 1200),        # a difference of exactly delta: reset, every time
                T_HALF: (1003, 1000, 1000, 1000, 1000),      # 0.33 * 1000 + 0.67 * 1003 + 0.5 = 1002.51 -> 1002
                T_TOP: (65500, 65535, 65535, 65535, 65535),  # stays at or below 65535
                T_NEVER: (0, 0, 0, 0, 0)}
    for p, values in designed.items():
        for f, val in zip(frames, values):
            f[p] = val
    out = [np.ascontiguousarray(f.reshape(T_SHAPE).astype(np.uint16)) for f in frames]
    for f in out:
        f.setflags(write=False)
    return out


def temporal_yardstick(frames, alpha=ALPHA, delta=DELTA):
    """[(output, state after)] per frame by a scalar loop from an all-zero state."""
    a = F32(alpha)
    oma = F32(1) - a
    state = np.zeros(frames[0].shape, np.uint16)
    res = []
    for frame in frames:
        out = np.zeros_like(state)
        new = state.copy()
        for v in range(frame.shape[0]):
            for u in range(frame.shape[1]):
                c, p = int(frame[v, u]), int(state[v, u])
                if c == 0:
                    continue
                o = c
                if p != 0 and abs(c - p) < delta:
                    f = a * F32(c)
                    g = oma * F32(p)
                    f = f + g
                    f = f + F32(0.5)
                    o = min(65535, int(f))
                out[v, u] = o
                new[v, u] = o
        state = new
        res.append((out, state))
    return res


# ---------------------------------------------------------------------------------------------------- the model's frame
def plane_frame(H=96, W=128):
    """A tilted plane from 0.2 m to 0.55 m with three raised blobs and some zero pixels."""
    rs = np.random.RandomState(12)
    v, u = np.mgrid[0:H, 0:W]
    z = 0.2 + 0.002 * u + 0.0012 * v
    for cv, cu in ((20, 30), (60, 90), (80, 20)):
        z = z - 0.03 * np.exp(-((v - cv) ** 2 + (u - cu) ** 2) / 40.0)
    d = np.round(z / SCALE).astype(np.uint16)
    d[rs.uniform(size=(H, W)) < 0.03] = 0
    d.setflags(write=False)
    return d, camera(H, W)
