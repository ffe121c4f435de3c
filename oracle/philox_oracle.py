"""A numpy twin of the Dropout mask of fc_end (rl_dropout_fwd / rl_dropout_bwd / rl_head_fwd / rl_head_bwd).

The mask is a pure function of (seed, key, element index): Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel Random
Numbers: As Easy as 1, 2, 3", SC'11) is evaluated once per four consecutive elements of the whole batch's (rows, C) tensor
and each of its four output words decides one element.  Written from the paper and the contract stated in the kernels'
header comments - uint64 arithmetic masked to 32 bits, no statistics anywhere - so that tests can name every keep bit.
Test infrastructure only: the product never imports oracle/."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_MUL_A = np.uint64(0xD2511F53)       # multiplies counter word 0
_MUL_B = np.uint64(0xCD9E8D57)       # multiplies counter word 2
_WEYL_0 = np.uint64(0x9E3779B9)      # golden ratio: added to key word 0 after every round
_WEYL_1 = np.uint64(0xBB67AE85)      # sqrt(3) - 1: added to key word 1
_S32 = np.uint64(32)


def _u64(v):
    return np.asarray(v, dtype=np.uint64)


def philox4x32_10(ctr4, key2):
    """Ten rounds of Philox-4x32.  ctr4: four words (each an array or a scalar, broadcast together), key2: two words.
    Returns the four output words as uint64 arrays holding 32-bit values.

    One round on (c0, c1, c2, c3) with key (k0, k1):
        hiA, loA = mulhilo(MUL_A, c0);  hiB, loB = mulhilo(MUL_B, c2)
        (c0, c1, c2, c3) <- (hiB ^ c1 ^ k0, loB, hiA ^ c3 ^ k1, loA)
    and the key is bumped by the two Weyl constants between rounds."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[_u64(c) & M32 for c in ctr4])
    k0, k1 = (_u64(k) & M32 for k in key2)
    for _ in range(10):
        a = _MUL_A * c0              # a 32 x 32 -> 64 bit product: exact in uint64
        b = _MUL_B * c2
        c0, c1, c2, c3 = (b >> _S32) ^ c1 ^ k0, b & M32, (a >> _S32) ^ c3 ^ k1, a & M32
        k0 = (k0 + _WEYL_0) & M32
        k1 = (k1 + _WEYL_1) & M32
    return c0, c1, c2, c3


def dropout_threshold(p) -> int:
    """A word keeps its element where word >= threshold: floor(p * 2^32) with p as the float32 the kernels receive,
    saturated so that it fits a 32-bit word."""
    return min(int(np.floor(np.float64(np.float32(p)) * 2.0 ** 32)), 2 ** 32 - 1)


def dropout_scale(p) -> np.float32:
    """What kept elements are multiplied by: 1 / (1 - p), both operations in float32."""
    return np.float32(1) / (np.float32(1) - np.float32(p))


def dropout_keep(seed: int, key: int, p, rows: int, C: int, first_row: int = 0) -> np.ndarray:
    """The keep decisions of rows [first_row, first_row + rows) of the whole batch's (., C) tensor: bool (rows, C).
    Quad q of the whole tensor (elements 4q .. 4q+3, row-major) takes the four output words of
    philox(counter = (lo32(q), hi32(q), lo32(key), hi32(key)), key = (lo32(seed), hi32(seed)))."""
    assert C % 4 == 0 and rows >= 0 and first_row >= 0
    seed, key = int(seed) & (2 ** 64 - 1), int(key) & (2 ** 64 - 1)
    first_quad = int(first_row) * C // 4
    assert first_quad + rows * C // 4 < 2 ** 64
    gq = np.uint64(first_quad) + np.arange(rows * C // 4, dtype=np.uint64)
    words = philox4x32_10((gq & M32, gq >> _S32, key & 0xFFFFFFFF, key >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    keep = np.stack(words, axis=-1) >= np.uint64(dropout_threshold(p))
    return keep.reshape(rows, C)


def keep_words(keep: np.ndarray) -> np.ndarray:
    """Head.mask's layout: for C = 32, one uint32 per row with bit c set where channel c is kept."""
    assert keep.ndim == 2 and keep.shape[1] == 32
    return (keep.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
