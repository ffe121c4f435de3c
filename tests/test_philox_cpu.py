"""oracle/philox_oracle.py - the numpy twin the Dropout kernels are compared with bit for bit (tests/test_dropout_gpu.py) -
against Random123's published known answers, and the properties of the mask that follow from its definition."""
import numpy as np
import pytest

from oracle import philox_oracle as PO

# Random123 (kat_vectors, philox4x32 10): counter, key, output, the words in philox4x32_10(ctr4, key2)'s order
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_known_answers(ctr, key, want):
    got = tuple(int(w) for w in PO.philox4x32_10(ctr, key))
    assert got == want, [hex(g) for g in got]


def test_known_answers_vectorised():
    """The three vectors as ONE call on arrays (the way dropout_keep calls it), next to unrelated counters."""
    for ctr, key, want in KAT:
        c = [np.array([7, w, 11], dtype=np.uint64) for w in ctr]
        got = PO.philox4x32_10(c, key)
        assert tuple(int(g[1]) for g in got) == want
        assert all(g.dtype == np.uint64 and int(g.max()) < 2 ** 32 for g in got)


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5, 0.8])
def test_keep_rate(p):
    """2^18 quads = 2^20 decisions: the kept fraction within 4 standard deviations of 1 - threshold / 2^32 (a condition on
    the twin - a `<` for the `>=`, or a threshold made from 1 - p, sits hundreds of deviations away except at p = 0.5)."""
    n = 1 << 20
    keep = PO.dropout_keep(5, 1, p, (1 << 18) // 8, 32)
    assert keep.shape == ((1 << 18) // 8, 32) and keep.dtype == np.bool_
    q = 1.0 - PO.dropout_threshold(p) / 2.0 ** 32
    sigma = np.sqrt(q * (1.0 - q) / n)
    dev = abs(float(keep.mean()) - q) / sigma
    print(f"[keep rate] p = {p}: {float(keep.mean()):.6f} vs {q:.6f}, {dev:.2f} sigma")
    assert dev < 4.0, (p, float(keep.mean()), q, dev)


def test_threshold_and_scale():
    assert PO.dropout_threshold(0.0) == 0
    assert PO.dropout_threshold(0.5) == 2 ** 31
    assert PO.dropout_threshold(0.25) == 2 ** 30
    assert PO.dropout_threshold(0.3) == int(np.floor(float(np.float32(0.3)) * 2 ** 32))      # the float32 p, not the double
    assert PO.dropout_threshold(0.3) != int(np.floor(0.3 * 2 ** 32))
    for p in (1.0, np.nextafter(np.float32(1), np.float32(0)), 0.99999999, 2.0):
        assert PO.dropout_threshold(p) <= 2 ** 32 - 1
    assert PO.dropout_threshold(1.0) == 2 ** 32 - 1
    assert PO.dropout_scale(0.5) == np.float32(2) and PO.dropout_scale(0.0) == np.float32(1)
    s = PO.dropout_scale(0.3)
    assert s.dtype == np.float32 and s == np.float32(1) / (np.float32(1) - np.float32(0.3))
    assert abs(float(s) - 1 / 0.7) < 1e-6 and abs(float(s) - 1 / 0.3) > 1.0


def test_a_word_equal_to_the_threshold_is_kept():
    """`>=`, not `>`: below p = 2^-8 every integer threshold under 2^24 is a float32 p, so a rate can be chosen whose
    threshold IS one of the generator's words.  That element is kept; one more and it is dropped."""
    q = np.arange(4096, dtype=np.uint64)
    words = np.stack(PO.philox4x32_10((q, 0, 1, 0), (5, 0)), axis=-1).reshape(-1)       # dropout_keep(5, 1, ., 512, 32)'s words
    hits = np.flatnonzero((words < (1 << 24)) & (words > 0))
    assert len(hits) > 8                                                                # (one word in 256)
    for e in hits[:8]:
        w = int(words[e])
        p = np.float32(w / 2.0 ** 32)
        assert PO.dropout_threshold(p) == w and float(p) * 2.0 ** 32 == w
        assert PO.dropout_keep(5, 1, p, 512, 32).reshape(-1)[e]
        p1 = np.float32((w + 1) / 2.0 ** 32)
        assert PO.dropout_threshold(p1) == w + 1
        assert not PO.dropout_keep(5, 1, p1, 512, 32).reshape(-1)[e]


def test_p_zero_keeps_everything():
    assert PO.dropout_keep(5, 1, 0.0, 64, 32).all()
    assert PO.dropout_keep(5 + (3 << 32), 1 << 40, 0.0, 3, 4, first_row=2 ** 31).all()


@pytest.mark.parametrize("C", [4, 32, 64])
def test_first_row_is_a_slice_of_the_whole_mask(C):
    whole = PO.dropout_keep(9, 4, 0.3, 1031, C)
    for first in (1, 700, 1030):
        np.testing.assert_array_equal(PO.dropout_keep(9, 4, 0.3, 1031 - first, C, first_row=first), whole[first:])


def test_high_counter_word_counts():
    """C = 32: eight quads per row, so row 2^29 starts at quad 2^32.  Rows around it: below, the high counter word is 0, from
    there on 1 - the rows from 2^29 on must differ from rows 0 .. (the same quads modulo 2^32), the rows below must equal
    the rows they are (no wrap-around)."""
    edge = 2 ** 29
    across = PO.dropout_keep(5, 1, 0.3, 8, 32, first_row=edge - 4)
    wrapped = PO.dropout_keep(5, 1, 0.3, 4, 32, first_row=0)
    assert (across[4:] != wrapped).any()
    assert abs(float((across[4:] != wrapped).mean()) - 2 * 0.3 * 0.7) < 0.2         # as different as two independent masks
    np.testing.assert_array_equal(across[:4], PO.dropout_keep(5, 1, 0.3, 4, 32, first_row=edge - 4))
    # ... and the same for the high words of key and seed
    base = PO.dropout_keep(5, 1, 0.3, 16, 32)
    assert (PO.dropout_keep(5 + (3 << 32), 1, 0.3, 16, 32) != base).any()
    assert (PO.dropout_keep(5, 1 + (1 << 32), 0.3, 16, 32) != base).any()
    assert (PO.dropout_keep(5, 2, 0.3, 16, 32) != base).any()


def test_keep_words_layout():
    keep = np.zeros((3, 32), dtype=bool)
    keep[0, 0] = keep[1, 31] = True
    keep[2, [1, 4, 9]] = True
    np.testing.assert_array_equal(PO.keep_words(keep), np.array([1, 1 << 31, (1 << 1) | (1 << 4) | (1 << 9)], dtype=np.uint32))
    k = PO.dropout_keep(5, 1, 0.3, 257, 32)
    w = PO.keep_words(k)
    assert w.dtype == np.uint32
    np.testing.assert_array_equal((w[:, None] >> np.arange(32, dtype=np.uint32)) & 1, k.astype(np.uint32))
