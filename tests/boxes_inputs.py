"""Shared inputs of the oriented-box tests (test_boxes_cpu.py, test_boxes_gpu.py): cases (xyz, ids, n_ids) from seeded
RandomStates - the smallest shapes at which csrc/boxes.hip can go wrong - and the twin's answer, computed once."""
import functools

import numpy as np

F32 = np.float32
L = 1024            # members per chunk of the fixed sums (utils/boxes.py: CHUNK)


def rotation(rs) -> np.ndarray:
    q, r = np.linalg.qr(rs.randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def blob(rs, n, offset=0.0, scale=1.0):
    """n points with standard deviations 4 : 2 : 1 along the columns of a random rotation, around a random centre."""
    R = rotation(rs)
    p = (rs.randn(n, 3) * np.array([4.0, 2.0, 1.0]) * scale) @ R.T + rs.uniform(-20, 20, 3) + offset
    return p.astype(F32), R


def blobs(sizes, seed, offset=0.0, shuffle=True, extra=0, dtype=np.int64):
    """One blob per entry of sizes (id = its position), `extra` points of id -1, in a seeded random order of the points."""
    rs = np.random.RandomState(seed)
    xyz = [blob(rs, n, offset)[0] for n in sizes] + [rs.uniform(-30, 30, (extra, 3)).astype(F32) + F32(offset)]
    ids = np.concatenate([np.full(n, k) for k, n in enumerate(sizes)] + [np.full(extra, -1)])
    xyz = np.concatenate(xyz)
    if shuffle:
        p = rs.permutation(ids.shape[0])
        xyz, ids = xyz[p], ids[p]
    return np.ascontiguousarray(xyz), ids.astype(dtype), None


def _build(name):
    if name == "single_point":                       # M = 1
        return np.array([[1.5, -2.0, 3.25]], F32), np.array([0]), None
    if name == "all_minus_one":
        xyz, ids, _ = blobs([4099], 1)
        return xyz, np.full_like(ids, -1), 3
    if name == "gaps":                               # ids 1, 4 and 9 of 14: empty ids before, between and after
        xyz, ids, _ = blobs([700, 1300, 2100], 2, extra=50)
        return xyz, np.where(ids >= 0, np.array([1, 4, 9])[np.maximum(ids, 0)], ids), 14
    if name == "short_segments":                     # around the wavefront
        return blobs([1, 2, 63, 64, 65], 3, extra=17)
    if name == "chunk_edges":                        # around the chunk
        return blobs([L - 1, L, L + 1, 2 * L + 1, 5 * L + 3], 4, extra=100)
    if name == "long_interleaved":                   # the long-segment path, and the stability of the sort
        small = np.random.RandomState(5).multinomial(50000 - 300, np.ones(300) / 300) + 1
        return blobs([150000] + small.tolist(), 5)
    if name == "duplicates":                         # every point three times, and one id of identical points
        xyz, ids, _ = blobs([300, 500], 6, shuffle=False)
        xyz, ids = np.tile(xyz, (3, 1)), np.tile(ids, 3)
        same = np.tile(np.array([[7.0, -3.5, 0.125]], F32), (1500, 1))
        p = np.random.RandomState(6).permutation(ids.shape[0] + 1500)
        return np.concatenate((xyz, same))[p], np.concatenate((ids, np.full(1500, 2)))[p], None
    if name == "flat_and_thin":                      # coplanar (axis-aligned and tilted) and collinear ids
        rs = np.random.RandomState(7)
        uv = rs.uniform(-8, 8, (1500, 2))
        plane0 = np.stack((uv[:, 0], uv[:, 1], np.full(1500, 2.5)), axis=1)
        plane1 = plane0 @ rotation(rs).T                        # (coplanar up to the rounding of the coordinates)
        t = rs.uniform(-10, 10, 1200)
        line0 = np.stack((np.full(1200, -1.0), t, np.full(1200, 4.0)), axis=1)
        line1 = np.outer(t, np.array([1.0, 2.0, -0.5])) + 3.0   # (exactly collinear: multiples of small binary fractions)
        two = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 12.0]])
        xyz = np.concatenate((plane0, plane1, line0, line1, two)).astype(F32)
        ids = np.concatenate((np.full(1500, 0), np.full(1500, 1), np.full(1200, 2), np.full(1200, 3), np.full(2, 4)))
        p = rs.permutation(ids.shape[0])
        return xyz[p], ids[p], None
    if name == "offset_1e4":
        return blobs([257, 1500, 3000], 8, offset=1e4, extra=30)
    if name == "int32_ids":
        return blobs([900, 2500, 40], 9, extra=11, dtype=np.int32)
    if name == "aniso":                              # well-conditioned axes: the cases of the independent oracle
        return blobs([256, 300, 1025, 4000], 10)
    if name == "aniso_far":
        return blobs([256, 2049, 700], 11, offset=1e4)
    raise KeyError(name)


CASES = ("single_point", "all_minus_one", "gaps", "short_segments", "chunk_edges", "long_interleaved", "duplicates",
         "flat_and_thin", "offset_1e4", "int32_ids", "aniso", "aniso_far")
ORACLE_CASES = ("aniso", "aniso_far", "offset_1e4", "chunk_edges")      # at least 256 points per id, deviations 4 : 2 : 1


@functools.lru_cache(maxsize=None)
def case(name):
    xyz, ids, n_ids = _build(name)
    for a in (xyz, ids):
        a.setflags(write=False)
    return xyz, ids, n_ids


@functools.lru_cache(maxsize=None)
def twin(name):
    from randlanet.utils.boxes import instance_boxes_host
    res = instance_boxes_host(*case(name))
    for a in res:
        a.setflags(write=False)
    return res


def assert_same(got, want, what=""):
    assert type(got).__name__ == "BoxResult" and got._fields == want._fields
    for field, a, b in zip(got._fields, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, field, a.dtype, b.dtype, a.shape, b.shape)
        if not np.array_equal(a, b):
            bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1))
            raise AssertionError(f"{what}: {field} differs at {bad.size} of {a.shape[0]} ids, first id {bad[0]}: "
                                 f"{a[bad[0]].tolist()} != {b[bad[0]].tolist()}")


def abi_refusals(lib, fake):
    """Every refusal of the rl_boxes_* entries: RL_ERR_ARGS and a message, before any launch (`fake` is a 256-byte aligned
    address that is never dereferenced)."""
    from randlanet import _hip
    E = _hip.ERR_ARGS
    M, I = 5000, 7
    need = lib.rl_boxes_workspace_bytes(M, I)
    assert need > 24 * M and lib.rl_boxes_workspace_bytes(2 ** 31 - 2, 1) > 24 * (2 ** 31 - 2)
    for m, i in ((0, I), (-1, I), (2 ** 31 - 1, I), (M, 0), (M, -3), (M, 2 ** 31 - 1)):
        assert lib.rl_boxes_workspace_bytes(m, i) == 0
    before = lib.rl_launch_count()
    sort = dict(ids=fake, id_bytes=8, M=M, I=I, ws=fake, ws_bytes=need, stream=None)
    moments = dict(xyz=fake, M=M, I=I, mean_out=None, cov_out=None, ws=fake, ws_bytes=need, stream=None)
    fit = dict(xyz=fake, M=M, I=I, count=fake, lo=fake, hi=fake, center=fake, axes=fake, extent=fake, lam=fake, ws=fake,
               ws_bytes=need, stream=None)
    for fn, good, name in ((lib.rl_boxes_sort, sort, b"rl_boxes_sort"), (lib.rl_boxes_moments, moments, b"rl_boxes_moments"),
                           (lib.rl_boxes_fit, fit, b"rl_boxes_fit")):
        bad = [("M", 0, b"M=0 outside"), ("M", 2 ** 31 - 1, b"outside 1 .. 2^31-2"), ("I", 0, b"I=0 ids"),
               ("I", 2 ** 31 - 1, b"ids, outside"), ("ws", None, b"null pointer"), ("ws", fake + 8, b"not 256-byte aligned"),
               ("ws_bytes", need - 1, b"workspace of"), ("ws_bytes", 0, b"workspace of"),
               ("I", I + 1000, b"workspace of")]                  # (more ids need more room)
        bad += [(k, None, b"null pointer") for k in good if k not in ("M", "I", "ws", "ws_bytes", "stream", "id_bytes",
                                                                        "mean_out", "cov_out")]
        if "id_bytes" in good:
            bad += [("id_bytes", 2, b"ids of 2 bytes"), ("id_bytes", 16, b"ids of 16 bytes")]
        for key, value, message in bad:
            args = dict(good)
            args[key] = value
            assert fn(*args.values()) == E, (name, key, value)
            err = lib.rl_last_error()
            assert name in err and message in err, (name, key, value, err)
    assert lib.rl_launch_count() == before
