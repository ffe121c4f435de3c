"""Shared inputs of the pair-count tests (test_instance_metrics_cpu.py, test_instance_metrics_gpu.py): cases (a, b, A, B)
from seeded RandomStates - the smallest shapes at which csrc/pairs.hip can go wrong - and the twin's answer, computed once."""
import functools

import numpy as np

CHUNK = 2048        # positions per chunk of the sort and the heads below 2^24 points


def _random(M, A, B, seed, lowest=-1, dtype=np.int64):
    rs = np.random.RandomState(seed)
    return rs.randint(lowest, A, M).astype(dtype), rs.randint(lowest, B, M).astype(dtype), A, B


def _sparse(M, A, B, seed, ids=40):
    """A few ids spread over the whole range of a wide key, the largest ones included."""
    rs = np.random.RandomState(seed)
    pool_a = np.concatenate(([-1, 0, A - 1], rs.randint(0, A, ids)))
    pool_b = np.concatenate(([-1, 0, B - 1], rs.randint(0, B, ids)))
    return pool_a[rs.randint(0, pool_a.size, M)], pool_b[rs.randint(0, pool_b.size, M)], A, B


def _build(name):
    if name.startswith("m_"):                        # sizes around the wavefront and the chunk edges
        M = int(name[2:])
        return _random(M, 7, 5, M)
    if name == "int32_70001":
        return _random(70001, 50, 40, 3, dtype=np.int32)
    if name == "mixed_dtypes":
        a, b, A, B = _random(4097, 300, 9, 4)
        return a.astype(np.int32), b.astype(np.int16), A, B
    if name == "million":
        return _random((1 << 20) + 3, 1000, 1000, 5)
    if name == "all_equal":                          # P = 1
        return np.full(5000, 3), np.full(5000, 2), 4, 6
    if name == "all_distinct":                       # P = M
        M = 5000
        p = np.random.RandomState(6).permutation(M)
        return p // 70, p % 70, 72, 70
    if name == "all_minus_one":
        return np.full(4099, -1), np.full(4099, -1), 3, 3
    if name == "below_minus_one":
        return _random(4100, 6, 6, 7, lowest=-5)
    if name == "long_runs":                          # sorted input, runs of 3000 that straddle the chunk edges
        k = np.arange(70001) // 3000
        return k // 5, k % 5, 5, 5
    # key widths: bits of (A + 1) * (B + 1) - 1.  With A, B >= 1 the narrowest key has 2 bits; "bit0" is that key with only
    # its lowest bit in use (a = -1 throughout)
    if name == "bits_2":
        return _random(4097, 1, 1, 8)
    if name == "bit0":
        a, b, A, B = _random(4097, 1, 1, 9)
        return np.full_like(a, -1), b, A, B
    if name == "bits_8":
        return _random(4097, 15, 15, 10)
    if name == "bits_9":
        return _random(4097, 15, 16, 11)
    if name == "bits_16":
        return _random(70001, 255, 255, 12)
    if name == "bits_17":
        return _random(70001, 255, 256, 13)
    if name == "bits_33":
        return _sparse(4097, 65535, 65536, 14)
    if name == "bits_41":                            # six digit passes
        return _sparse(70001, 1 << 20, 1 << 20, 15)
    if name == "bits_37_high_only":                  # B + 1 = 2^16 and a + 1 in steps of 2^16: keys that differ above bit 32 only
        rs = np.random.RandomState(16)
        a = (rs.randint(0, 16, 4097) << 16) - 1
        return a, np.full(4097, 5), 1 << 20, (1 << 16) - 1
    raise KeyError(name)


WIDTHS = {"bits_2": 2, "bit0": 2, "bits_8": 8, "bits_9": 9, "bits_16": 16, "bits_17": 17, "bits_33": 33, "bits_41": 41,
          "bits_37_high_only": 37}
CASES = (["m_1", "m_63", "m_64", "m_65", "m_2047", "m_2048", "m_2049", "m_4097", "m_70001", "int32_70001", "mixed_dtypes",
          "million", "all_equal", "all_distinct", "all_minus_one", "below_minus_one", "long_runs"] + list(WIDTHS))
SMALL = [c for c in CASES if c not in ("million", "bits_33", "bits_41", "bits_37_high_only")]      # a dense table fits


@functools.lru_cache(maxsize=None)
def case(name):
    a, b, A, B = _build(name)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b, int(A), int(B)


@functools.lru_cache(maxsize=None)
def twin(name):
    from randlanet.utils.instance_metrics import pair_counts_host
    res = pair_counts_host(*case(name))
    for r in res:
        r.setflags(write=False)
    return res


def brute(name):
    """The dense (A + 1, B + 1) table by np.add.at, and its non-zero entries in row-major order."""
    a, b, A, B = case(name)
    table = np.zeros((A + 1, B + 1), np.int64)
    np.add.at(table, (np.maximum(a.astype(np.int64), -1) + 1, np.maximum(b.astype(np.int64), -1) + 1), 1)
    pa, pb = np.nonzero(table)
    return pa - 1, pb - 1, table[pa, pb]


def assert_same(got, want, what=""):
    for g, w, n, dt in zip(got, want, ("pa", "pb", "count"), (np.int32, np.int32, np.int64)):
        assert g.dtype == dt and w.dtype == dt, f"{what} {n}: dtypes {g.dtype}, {w.dtype}"
        assert np.array_equal(g, w), f"{what} {n} differs"
