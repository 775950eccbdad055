"""CPU: the scalar definition of compress_mode 2 ("high") against a dictionary (tests/sim/high_dict_model.c): without a dictionary it
is high_encoder_model.c; with one its blocks decode through the oracle's dictionary decoder to the input and are smaller than both the
oracle's compress_with_dict and the high model without a dictionary; the known answers at depth 16 are pinned."""
import random

import pytest

import hc_dict_model as D
import hc_model as H
import oracle_api as O


def J():
    return O.fixture_plain("compression_66k_JSON")


def T():
    return O.fixture_plain("compression_65k")


def roundtrip(data, d, comp):
    assert len(comp) <= O.max_out(len(data))
    assert O.decompress(comp, len(data), dict_data=d if d else None) == ("ok", data)


def test_no_dictionary_is_the_plain_model():
    j = J()
    for data in (b"", j[:11], j[:13], j[:4096], j, (j * 3)[:150000]):
        for d in (b"", j[:1], j[:2], j[:3]):
            for depth in (1, 16):
                assert D.compress(data, d, depth) == H.compress(data, depth), (len(data), len(d), depth)


KNOWN = [
    ("j", slice(40000, 44096), slice(0, 4096), 1145, 1007),
    ("j", slice(40000, 44096), slice(0, 32768), 1145, 604),
    ("j", slice(40000, 44096), slice(0, 40000), 1145, 601),
    ("j", slice(50000, 50100), slice(0, 32768), 84, 15),
    ("j", slice(41000, None), slice(0, 32768), 4498, 3751),
    ("j", slice(40000, 40013), slice(0, 32768), 14, 9),
    ("t", slice(40000, 44096), slice(0, 32768), 2787, 1799),
    ("t", slice(41000, None), slice(0, 40000), 13191, 11050),
]


@pytest.mark.parametrize("k", range(len(KNOWN)))
def test_known_answers(k):
    src, blk, dct, plain, with_dict = KNOWN[k]
    s = J() if src == "j" else T()
    data, d = s[blk], s[dct]
    assert len(H.compress(data, 16)) == plain
    comp = D.compress(data, d, 16)
    roundtrip(data, d, comp)
    assert len(comp) == with_dict


def test_known_answer_three_chunks():
    j = J()
    data, d = (j * 3)[:150000], j[100:30000]
    assert len(H.compress(data, 16)) == 29527
    comp = D.compress(data, d, 16)
    roundtrip(data, d, comp)
    assert len(comp) == 22091


def test_24_cases_against_the_oracle_and_no_dictionary():
    total = oracle_total = plain_total = 0
    for s in (J(), T()):
        for dl in (4096, 32768, 40000):
            for blk in (slice(40000, 44096), slice(50000, 50100), slice(41000, None), slice(40000, 40013)):
                data, d = s[blk], s[:dl]
                comp = D.compress(data, d, 16)
                roundtrip(data, d, comp)
                o, p = len(O.compress_with_dict(data, d)), len(H.compress(data, 16))
                assert len(comp) <= o and len(comp) <= p, (dl, blk, len(comp), o, p)
                total += len(comp); oracle_total += o; plain_total += p
    print("high with dictionary %d, oracle with dictionary %d, high without %d" % (total, oracle_total, plain_total))
    assert (total, oracle_total, plain_total) == (54767, 67576, 65502)
    assert total < oracle_total and total < plain_total


def sequences(comp):
    """(literals, offset, match length) of every sequence but the last"""
    i, out = 0, []
    while True:
        t = comp[i]; i += 1
        lit = t >> 4
        if lit == 15:
            while True:
                b = comp[i]; i += 1; lit += b
                if b != 255:
                    break
        i += lit
        if i >= len(comp):
            return out
        off = comp[i] | comp[i + 1] << 8
        i += 2
        ml = (t & 15) + 4
        if (t & 15) == 15:
            while True:
                b = comp[i]; i += 1; ml += b
                if b != 255:
                    break
        out.append((lit, off, ml))


def test_match_from_the_dictionary_into_the_block():
    rnd = random.Random(5)
    d = bytes(rnd.getrandbits(8) for _ in range(5000))
    tail = d[-40:]
    # the block repeats the dictionary's last 40 bytes twice: its first match starts 40 bytes in front of the block and runs on
    # through the block's own first copy
    data = tail + tail + bytes(rnd.getrandbits(8) for _ in range(30))
    comp = D.compress(data, d, 16)
    roundtrip(data, d, comp)
    assert sequences(comp)[0] == (0, 40, 80)


def test_offset_65532():
    rnd = random.Random(6)
    d = bytes(rnd.getrandbits(8) for _ in range(32768))
    data = bytes(rnd.getrandbits(8) for _ in range(32764)) + d[:4] + bytes(rnd.getrandbits(8) for _ in range(40))
    comp = D.compress(data, d, 16)
    roundtrip(data, d, comp)
    seqs = sequences(comp)
    assert (32764, 65532, 4) in seqs, seqs
    # one byte more in front and the position lies in chunk 1, which does not see the dictionary
    data = b"\x00" + data
    comp = D.compress(data, d, 16)
    roundtrip(data, d, comp)
    assert all(off != 65533 for _, off, _ in sequences(comp))


DICT_LENS = (0, 3, 4, 5, 100, 4096, 32767, 32768, 32769, 70000)
BLOCK_LENS = (0, 1, 11, 12, 13, 100, 4096, 32767, 32768, 32769, 40000, 65536, 65537)


def test_fuzz_through_the_oracles_decoder():
    rnd = random.Random(99)
    j, t = J(), T()
    noise = bytes(rnd.getrandbits(8) for _ in range(70000))
    pool = (j * 3, t * 3, noise * 3, bytes(200000), (bytes(range(256)) * 800))
    for _ in range(400):
        dl, n, depth = rnd.choice(DICT_LENS), rnd.choice(BLOCK_LENS), rnd.choice((1, 4, 16, 64))
        src = rnd.choice(pool)
        at = rnd.randrange(0, 1000)
        d = src[at:at + dl]
        other = rnd.choice(pool) if rnd.random() < 0.2 else src
        at2 = rnd.randrange(0, len(other) - n)
        data = other[at2:at2 + n]
        comp = D.compress(data, d, depth)
        assert len(comp) <= O.max_out(n)
        assert O.decompress(comp, n, dict_data=d if d else None) == ("ok", data), (dl, n, depth)
