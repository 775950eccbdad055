"""CPU test of the filters' numpy model (tests/filter_model.py), the definition the kernels of lz4_filter.hip are checked against: the
inverse undoes the forward transform for every small length, hand-written known answers, and the reason for the feature -- numeric data
compresses far better behind a filter -- as two conditions through the oracle's encoder."""
import numpy as np
import pytest

import filter_model as M
import oracle_api as O

SIZES = list(range(301)) + [1023, 1024, 1025, 4093, 65536, 65537, 100003]


@pytest.mark.parametrize("E", M.ELEMS)
def test_inverse_of_forward_is_identity(E):
    rnd = np.random.default_rng(E)
    for L in SIZES:
        x = rnd.integers(0, 256, L, dtype=np.uint8)
        for filt in (M.NONE, M.SHUFFLE, M.BITSHUFFLE):
            y = M.forward(x, filt, E)
            assert y.size == L and y.dtype == np.uint8
            assert (M.inverse(y, filt, E) == x).all(), (filt, E, L)
            assert (M.forward(M.inverse(x, filt, E), filt, E) == x).all(), (filt, E, L)
            assert np.array_equal(np.sort(y), np.sort(x)) or filt == M.BITSHUFFLE            # (a byte permutation; bitshuffle permutes bits)
            assert int(np.unpackbits(y).sum()) == int(np.unpackbits(x).sum())


def test_the_tail_stays_where_it_is():
    x = np.arange(200, 200 + 37, dtype=np.uint8)
    for E in M.ELEMS:
        m, m8 = 37 // E, 37 // E // 8 * 8
        assert (M.shuffle(x, E)[m * E:] == x[m * E:]).all()
        assert (M.bitshuffle(x, E)[m8 * E:] == x[m8 * E:]).all()
    assert (M.shuffle(x, 1) == x).all()
    for L in range(8):                                   # fewer than 8 elements: nothing to transpose
        assert (M.bitshuffle(x[:L], 1) == x[:L]).all()


def test_definition_index_by_index():
    """the two formulas of the definition, one output byte / bit at a time"""
    rnd = np.random.default_rng(5)
    for E in M.ELEMS:
        L = 16 * E * 3 + E - 1 + (E > 1)
        x = rnd.integers(0, 256, L, dtype=np.uint8)
        m = L // E
        y = M.shuffle(x, E)
        for e in range(m):
            for j in range(E):
                assert y[j * m + e] == x[e * E + j]
        m8 = m // 8 * 8
        z = M.bitshuffle(x, E)
        for j in range(E):
            for k in range(8):
                p = 8 * j + k
                for q in range(m8 // 8):
                    for b in range(8):
                        assert (z[p * m8 // 8 + q] >> b) & 1 == (x[(8 * q + b) * E + j] >> k) & 1


def test_known_answers():
    assert M.shuffle(bytes(range(7)), 2).tolist() == [0, 2, 4, 1, 3, 5, 6]
    assert M.unshuffle(bytes([0, 2, 4, 1, 3, 5, 6]), 2).tolist() == list(range(7))
    # E = 1, 8 elements and one byte behind them: only element 0 has bit 0 set -> plane 0 = 01, planes 1 - 7 = 00, then the tail
    assert M.bitshuffle(bytes([1, 0, 0, 0, 0, 0, 0, 0, 0x7F]), 1).tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0x7F]
    assert M.bitshuffle(bytes([0x80] * 8), 1).tolist() == [0] * 7 + [0xFF]
    assert M.bitshuffle(bytes([0, 0, 0, 0x04, 0, 0, 0, 0]), 1).tolist() == [0, 0, 0x08, 0, 0, 0, 0, 0]      # element 3, bit 2 -> plane 2, bit 3
    # E = 2, the 16 elements 0 .. 15 as LE u16: m8 = 16, 16 planes of 2 bytes (q = 0: elements 0 - 7, q = 1: elements 8 - 15).
    #   byte 0 of element e is e, byte 1 is 0, so planes 8 - 15 (byte 1) and planes 4 - 7 (bits 4 - 7 of e < 16) are zero;
    #   plane 0 = bit 0 of e: set for odd e -> bits 1, 3, 5, 7 of both bytes: AA AA
    #   plane 1 = bit 1 of e: e = 2, 3, 6, 7 and 10, 11, 14, 15 -> bits 2, 3, 6, 7 of both bytes: CC CC
    #   plane 2 = bit 2 of e: e = 4 - 7 and 12 - 15 -> bits 4 - 7 of both bytes: F0 F0
    #   plane 3 = bit 3 of e: e = 8 - 15 -> nothing in q = 0, everything in q = 1: 00 FF
    x = np.arange(16, dtype="<u2").view(np.uint8)
    want = [0xAA, 0xAA, 0xCC, 0xCC, 0xF0, 0xF0, 0x00, 0xFF] + [0] * 24
    assert M.bitshuffle(x, 2).tolist() == want
    assert (M.unbitshuffle(bytes(want), 2) == x).all()


def test_filters_are_the_reason_numeric_data_compresses():
    """64 KiB of seeded numeric data through the oracle's compress (measured with liblz4 1.9.3: bf16 0.758 bit-shuffled against 1.004 raw,
    int64 timestamps 0.214 byte-shuffled against 0.626 raw)"""
    bf16 = M.bf16_weights(65536, 20)
    raw, shuffled = len(O.compress(bf16.tobytes())), len(O.compress(M.bitshuffle(bf16, 2).tobytes()))
    print("bf16 N(0, 0.02): raw %d, bit-shuffled %d (%.3f of raw)" % (raw, shuffled, shuffled / raw))
    assert shuffled <= 0.85 * raw
    ts = M.int64_timestamps(65536, 21)
    raw, shuffled = len(O.compress(ts.tobytes())), len(O.compress(M.shuffle(ts, 8).tobytes()))
    print("int64 timestamps: raw %d, byte-shuffled %d (%.3f of raw)" % (raw, shuffled, shuffled / raw))
    assert shuffled <= 0.5 * raw
