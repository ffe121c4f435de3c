"""Shared inputs and yardsticks of the TSDF tests (test_tsdf_*): the cameras, analytically rendered and seeded synthetic
frames, the volumes at which the kernels can still go wrong, hand-planted states for the extraction, scalar restatements of the
contract that are independent of the package's vectorised twin (np.float32 scalars, one operation per statement, in the order
of utils/tsdf.py's docstring), and the twin's result per case (computed once, never modified).

A case is Case(dims, origin, voxel, trunc, max_weight, camera, z_range, frames [(depth, pose or None), ...], min_weight)."""
from collections import namedtuple

import numpy as np

F32 = np.float32
SCALE = 0.00025
Z_RANGE = (0.05, 0.6)
Case = namedtuple("Case", ["dims", "origin", "voxel", "trunc", "max_weight", "camera", "z_range", "frames", "min_weight"])
_cases, _twins, _planted, _planted_twins = {}, {}, {}, {}

SMALL, LARGE, ODD = (36, 48), (72, 96), (3, 67)            # H x W of the frames


def camera(H, W, scale=SCALE):
    """Intrinsics that are deliberately not round, so every rounding matters; about 47 degrees across."""
    from randlanet.utils.depth import DepthCamera
    return DepthCamera(W, H, 1.15 * W + 0.5, 1.15 * W + 1.25, W / 2 - 0.2, H / 2 + 0.3, scale)


def pose(rx=0.0, ry=0.0, rz=0.0, t=(0.0, 0.0, 0.0)):
    """A camera-to-world transform (4, 4) float64 from three angles in degrees and a translation."""
    ax, ay, az = np.deg2rad([rx, ry, rz])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


# ------------------------------------------------------------------------------------------------------------ the frames
def tilted_frame(H, W, seed, z0=0.3, du=0.0012, dv=-0.0007, scale=SCALE):
    """A tilted plane around z0 with a tenth of holes and a twentieth of pixels beyond z_hi."""
    rs = np.random.RandomState(seed)
    v, u = np.mgrid[0:H, 0:W]
    z = z0 + du * (u - W / 2) * (48.0 / W) + dv * (v - H / 2) * (36.0 / H)
    d = np.round(z / scale).astype(np.uint16)
    d[rs.uniform(size=(H, W)) < 0.1] = 0
    d[rs.uniform(size=(H, W)) < 0.05] = 2600                  # 0.65 m: outside z_range
    d.setflags(write=False)
    return d


SPHERE_C, SPHERE_R, GROUND_Y = np.array([0.0, 0.0, 0.35]), 0.08, 0.1


def render(H, W, T, ground=False):
    """The depth frame (H, W) uint16 of the sphere of radius 0.08 at (0, 0, 0.35) - and with `ground` the plane y = 0.1 under
    it - seen from the camera-to-world pose T, by analytic ray casting in float64; 0 where a ray hits nothing."""
    cam = camera(H, W)
    v, u = np.mgrid[0:H, 0:W]
    d_cam = np.stack(((u - float(cam.ppx)) / float(cam.fx), (v - float(cam.ppy)) / float(cam.fy), np.ones((H, W))), axis=-1)
    d_w = d_cam @ T[:3, :3].T                                 # (per unit of camera z: the ray parameter IS the depth)
    o = T[:3, 3]
    oc = o - SPHERE_C
    a = (d_w * d_w).sum(-1)
    b = 2.0 * (d_w @ oc)
    c = oc @ oc - SPHERE_R ** 2
    disc = b * b - 4 * a * c
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
        if ground:
            zg = (GROUND_Y - o[1]) / d_w[..., 1]
            z = np.minimum(z, np.where(zg > 0, zg, np.inf))
    d = np.where(np.isfinite(z) & (z > 0) & (z < 65535 * SCALE), np.round(z / SCALE), 0).astype(np.uint16)
    d.setflags(write=False)
    return d


SPHERE_POSES = (pose(), pose(ry=14.0, t=(-0.085, 0.0, 0.012)), pose(rx=-12.0, ry=-9.0, t=(0.055, -0.075, 0.01)))
# (pitch, roll, height and depth: the sphere on its plane does not determine a turn about the plane's normal through the centre)
TRACK_POSES = (pose(), pose(rx=2.0, rz=1.5, t=(0.002, 0.01, 0.008)), pose(rx=4.0, rz=3.0, t=(0.004, 0.02, 0.016)))


def sphere_case(ground=False, poses=SPHERE_POSES):
    H, W = LARGE
    frames = [(render(H, W, T, ground), T) for T in poses]
    return Case((32, 32, 32), (-0.16, -0.16, 0.19), 0.01, None, 64, camera(H, W), Z_RANGE, frames, 1)


# -------------------------------------------------------------------------------------------------------------- the cases
# the volumes: a single voxel; no dimension a multiple of 4; a single short row; 1023, 1024 and 1025 voxels around the chunk
# boundary; a general small one; more chunks than the scan's workgroup has threads (GR_THREADS = 256: 1280 chunks here)
DIMS = ((1, 1, 1), (5, 3, 2), (7, 1, 1), (33, 31, 1), (32, 32, 1), (41, 25, 1), (13, 11, 9), (128, 128, 80))
CASES = tuple("x".join(map(str, d)) for d in DIMS) + (
    "outside", "behind", "centre-plane", "borders", "trunc-edges", "saturate", "sphere", "odd-frame")
SCALAR = ("1x1x1", "5x3x2", "7x1x1", "13x11x9", "behind", "centre-plane", "borders", "trunc-edges", "saturate", "outside")


def _centred(dims, voxel, z=0.3):
    """The origin that centres a volume of `dims` voxels on the optical axis at depth z."""
    return tuple(float(c - 0.5 * n * voxel) for c, n in zip((0.003, -0.002, z), dims))


def _build(name):
    H, W = SMALL
    cam = camera(H, W)
    two = [(tilted_frame(H, W, 11), None), (tilted_frame(H, W, 12, 0.302, -0.0009, 0.0011), pose(2.0, -3.0, 1.0, (0.01, -0.004, 0.003)))]
    if name[0].isdigit():
        dims = tuple(int(s) for s in name.split("x"))
        if dims == (128, 128, 80):
            Hl, Wl = LARGE
            frames = [(tilted_frame(Hl, Wl, 13), None), (tilted_frame(Hl, Wl, 14, 0.305, -0.001, 0.0009), two[1][1])]
            return Case(dims, _centred(dims, 0.002), 0.002, None, 64, camera(Hl, Wl), Z_RANGE, frames, 1)
        voxel = 0.19 / max(dims) if max(dims) > 1 else 0.01           # the volume fills most of the frame's width
        return Case(dims, _centred(dims, voxel), voxel, 0.02 if dims[2] == 1 else None, 64, cam, Z_RANGE, two, 1)
    if name == "outside":            # wholly outside the frustum, to the side; and a frame that sees it far behind its surface
        return Case((13, 11, 9), (5.0, -0.05, 0.2), 0.01, None, 64, cam, Z_RANGE, [two[0], (two[0][0], pose(ry=180.0, t=(5.0, 0, 2.0)))], 1)
    if name == "behind":             # the camera's plane z = 0 cuts the volume: q_z <= 0 for its near layers
        return Case((13, 11, 9), (-0.2, -0.17, -0.22), 0.07, 0.1, 64, cam, Z_RANGE, two, 1)
    if name == "centre-plane":
        # c_z = -0.5 + 0.5 * 1 = 0 exactly, and the pose puts the camera 2e-38 behind it: q_z = 2e-38 (a normal float32), so
        # uf and vf overflow to + or - infinity wherever c_x, c_y = -4 .. 4 are not 0, and the one voxel with c_x = c_y = 0
        # reads the pixel at the principal point
        T = pose(t=(0.0, 0.0, -2e-38))
        return Case((9, 7, 1), (-4.5, -3.5, -0.5), 1.0, None, 64, cam, Z_RANGE, [(two[0][0], T)], 1)
    if name == "borders":            # a slab at 0.3 m wider than the frustum, its voxels closer than the pixels: they
        #                              project onto every pixel of the first and last row and column, and beyond them
        return Case((71, 53, 1), _centred((71, 53, 1), 0.004), 0.004, 0.02, 64, cam, Z_RANGE, [two[0]], 1)
    if name == "trunc-edges":
        # powers of two throughout: c_z = 0.25 + (k - 6) / 128 and z = 1024 / 4096 = 0.25 exactly, trunc = 1 / 32, so
        # sdf = -trunc exactly at k = 10 (kept), below it at k = 11, 12 (skipped), above +trunc at k = 0, 1 (clamped to 1)
        frame = np.full((H, W), 1024, np.uint16)
        frame.setflags(write=False)
        return Case((3, 3, 13), (-1.5 / 128, -1.5 / 128, 0.25 - 6.5 / 128), 1.0 / 128, None, 64, camera(H, W, 1.0 / 4096), Z_RANGE,
                    [(frame, None)], 1)
    if name == "saturate":           # the same frame max_weight + 3 times at max_weight = 2
        return Case((5, 3, 2), _centred((5, 3, 2), 0.03), 0.03, None, 2, cam, Z_RANGE, [two[0]] * 5, 2)
    if name == "sphere":
        return sphere_case()
    if name == "odd-frame":          # 3 x 67: frame 1 of a (2, H, W) tensor is only 2-byte aligned
        Ho, Wo = ODD
        rs = np.random.RandomState(5)
        frames = [(np.ascontiguousarray(rs.randint(1000, 1400, (Ho, Wo)).astype(np.uint16)), None) for _ in range(2)]
        return Case((13, 11, 9), _centred((13, 11, 9), 0.012), 0.012, None, 64, camera(Ho, Wo), Z_RANGE, frames, 1)
    raise KeyError(name)


def case(name):
    if name not in _cases:
        _cases[name] = _build(name)
    return _cases[name]


def volume(c: Case, device="cpu"):
    from randlanet.utils.tsdf import TsdfVolume
    return TsdfVolume(c.origin, c.voxel, c.dims, c.trunc, c.max_weight, device=device)


def twin(name):
    """[(tsdf, weight) after every frame], TsdfCloud at the case's min_weight: the numpy twin, computed once."""
    if name not in _twins:
        c = case(name)
        vol = volume(c)
        states = []
        for depth, T in c.frames:
            vol.integrate(depth, c.camera, T, c.z_range)
            states.append((vol.tsdf.copy(), vol.weight.copy()))
        cloud = vol.extract(c.min_weight)
        for a in [x for s in states for x in s] + list(cloud):
            a.setflags(write=False)
        _twins[name] = (states, cloud)
    return _twins[name]


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    assert a.dtype == np.float32, a.dtype
    return a.view(np.uint32)


def assert_same_state(got, want, what=""):
    for g, w, n in zip(got, want, ("tsdf", "weight")):
        assert tuple(g.shape) == w.shape, (what, n)
        assert np.array_equal(bits(g), bits(w)), (what, n, int((bits(g) != bits(w)).sum()))


def assert_same_cloud(got, want, what=""):
    gx, ge = (np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a) for a in got)
    assert gx.dtype == np.float32 and ge.dtype == np.int64, what
    assert gx.shape == want.xyz.shape and ge.shape == want.edge.shape and gx.shape == (ge.shape[0], 3), (what, gx.shape, want.xyz.shape)
    assert np.array_equal(ge, want.edge), what
    assert np.array_equal(gx.view(np.uint32), want.xyz.view(np.uint32)), what


# ---------------------------------------------------------------------------------------------- hand-planted states
PLANTED = ("designed", "random-5x3x2", "random-7x1x1", "random-1x1x1", "random-33x31x1", "random-32x32x1", "random-41x25x1",
           "random-13x11x9", "random-128x128x80")
PLANTED_SCALAR = ("designed", "random-5x3x2", "random-7x1x1", "random-1x1x1", "random-13x11x9")
# voxel (i, j, k) of the designed state -> what it is there for
P_ALL3, P_LAST, P_F0, P_F1, P_ZEROS, P_NEGZERO, P_LIGHT = (1, 1, 0), (4, 2, 1), (3, 0, 0), (0, 2, 1), (2, 0, 1), (0, 0, 0), (3, 2, 0)


def planted(name):
    """(tsdf, weight (nz, ny, nx) float32, origin, voxel, min_weight, max_weight) of a state written by hand."""
    if name in _planted:
        return _planted[name]
    if name == "designed":
        nx, ny, nz = 5, 3, 2
        t = np.full((nz, ny, nx), 0.5, F32)
        w = np.full((nz, ny, nx), 2.0, F32)
        t[P_ALL3[::-1]] = -0.25                      # negative among positives: emits on x, y and z (and its lower
        #                                              neighbours emit towards it)
        t[P_LAST[::-1]] = -0.75                      # the last voxel on every axis: no neighbour of its own
        t[P_F0[::-1]] = 0.0                          # 0.0 against a negative neighbour one up in x: f = 0
        t[0, 0, 4] = -0.5
        t[P_F1[::-1]] = -0.5                         # negative against 0.0 one up in x: f = 1
        t[1, 2, 1] = 0.0
        t[P_ZEROS[::-1]] = 0.0                       # both exactly 0 along x: no point there
        t[1, 0, 3] = 0.0
        t[P_NEGZERO[::-1]] = -0.0                    # -0.0 is not below 0: no crossing against the 0.5 around it
        t[0, 2, 3] = -0.5                            # P_LIGHT: crossings around a voxel just below min_weight - no point,
        w[0, 2, 3] = np.nextafter(F32(2.0), F32(0))  # as voxel n or as neighbour b; the negative voxel (4, 2, 0) next to it
        t[0, 2, 4] = -0.5                            # weighs exactly min_weight: (4, 1, 0) emits towards it along y
        res = (t, w, (0.1, -0.2, 0.3), 0.01, 2, 64)
    else:
        dims = tuple(int(s) for s in name.split("-")[1].split("x"))
        nx, ny, nz = dims
        rs = np.random.RandomState(sum(dims))
        if nx * ny * nz > 1 << 16:                   # smooth, so that a small share of the edges emit, in every chunk
            k, j, i = np.mgrid[0:nz, 0:ny, 0:nx]
            t = (np.sin(i * 0.11 + j * 0.05) + np.sin(k * 0.2 + j * 0.13) + 0.3 * rs.uniform(-1, 1, (nz, ny, nx))).astype(F32) * F32(0.4)
        else:
            t = rs.uniform(-1, 1, (nz, ny, nx)).astype(F32)
        w = rs.randint(0, 4, (nz, ny, nx)).astype(F32)
        res = (t, w, (-0.3, 0.2, 0.1), 0.0125, 2, 64)
    for a in res[:2]:
        a.setflags(write=False)
    _planted[name] = res
    return res


def planted_twin(name):
    if name not in _planted_twins:
        from randlanet.utils.tsdf import extract_host
        t, w, origin, voxel, min_weight, _ = planted(name)
        cloud = extract_host(t, w, tuple(F32(o) for o in origin), F32(voxel), min_weight)
        for a in cloud:
            a.setflags(write=False)
        _planted_twins[name] = cloud
    return _planted_twins[name]


# ------------------------------------------------------------------------------------------------- scalar restatements
def scalar_w2c(T):
    """The twelve float32 of the contract, element by element."""
    T = np.eye(4) if T is None else np.asarray(T, np.float64)
    out = []
    for a in range(3):
        out += [T[b, a] for b in range(3)]                                   # R' = R^T, row a
    for a in range(3):
        out.append(-(T[0, a] * T[0, 3] + T[1, a] * T[1, 3] + T[2, a] * T[2, 3]))
    return [F32(x) for x in out]


def _centre(o, i, voxel):
    c = F32(i) + F32(0.5)
    c = c * voxel
    return o + c


def scalar_integrate(tsdf, weight, c: Case, depth, T, hits=None):
    """One frame into tsdf and weight (nz, ny, nx) float32 in place, by a per-voxel loop written from the contract.  hits: a
    set that receives the (v, u) of every pixel a voxel read."""
    nx, ny, nz = c.dims
    cam = c.camera
    H, W = depth.shape
    ox, oy, oz = (F32(o) for o in c.origin)
    voxel = F32(c.voxel)
    trunc = F32(4) * voxel if c.trunc is None else F32(c.trunc)
    z_lo, z_hi = F32(c.z_range[0]), F32(c.z_range[1])
    r = scalar_w2c(T)
    mw = F32(c.max_weight)
    with np.errstate(all="ignore"):
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    cx, cy, cz = _centre(ox, i, voxel), _centre(oy, j, voxel), _centre(oz, k, voxel)
                    q = []
                    for a in range(3):
                        p0 = r[3 * a] * cx
                        p1 = r[3 * a + 1] * cy
                        s = p0 + p1
                        p2 = r[3 * a + 2] * cz
                        s = s + p2
                        q.append(s + r[9 + a])
                    if not q[2] > 0:
                        continue
                    uf = q[0] / q[2]
                    uf = uf * cam.fx
                    uf = uf + cam.ppx
                    uf = uf + F32(0.5)
                    vf = q[1] / q[2]
                    vf = vf * cam.fy
                    vf = vf + cam.ppy
                    vf = vf + F32(0.5)
                    if not (uf >= 0 and uf < F32(W) and vf >= 0 and vf < F32(H)):
                        continue
                    u, v = int(uf), int(vf)
                    if hits is not None:
                        hits.add((v, u))
                    d = int(depth[v, u])
                    if d == 0:
                        continue
                    z = F32(d) * cam.depth_scale
                    if not (z_lo < z and z < z_hi):
                        continue
                    sdf = z - q[2]
                    if sdf < -trunc:
                        continue
                    s = sdf / trunc
                    if s > F32(1):
                        s = F32(1)
                    w = weight[k, j, i]
                    t = tsdf[k, j, i] * w
                    t = t + s
                    w1 = w + F32(1)
                    tsdf[k, j, i] = t / w1
                    weight[k, j, i] = min(w1, mw)


def scalar_extract(tsdf, weight, origin, voxel, min_weight):
    """(xyz (M, 3) float32, edge (M,) int64) by a per-voxel loop written from the contract."""
    nz, ny, nx = tsdf.shape
    o = [F32(x) for x in origin]
    voxel = F32(voxel)
    xyz, edge = [], []
    mw = F32(min_weight)
    with np.errstate(all="ignore"):
        for n in range(nx * ny * nz):
            i, j, k = n % nx, (n // nx) % ny, n // (nx * ny)
            for a, (inside, b) in enumerate(((i + 1 < nx, (k, j, i + 1)), (j + 1 < ny, (k, j + 1, i)), (k + 1 < nz, (k + 1, j, i)))):
                if not inside:
                    continue
                tn, tb = tsdf[k, j, i], tsdf[b]
                if not (weight[k, j, i] >= mw and weight[b] >= mw and (tn < 0) != (tb < 0)):
                    continue
                den = tn - tb
                f = tn / den
                p = [_centre(o[0], i, voxel), _centre(o[1], j, voxel), _centre(o[2], k, voxel)]
                step = f * voxel
                p[a] = p[a] + step
                xyz.append(p)
                edge.append(3 * n + a)
    return np.array(xyz, F32).reshape(-1, 3), np.array(edge, np.int64)
