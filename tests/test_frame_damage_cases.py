"""CPU: the census of tests/frame_damage_cases.py against the oracle alone -- the generator must not quietly degenerate into frames
that all fail the same way."""
import collections

import pytest

import frame_damage_cases as D

OUTPUT_TOO_SMALL = 1
DECOMPRESSION, IO, BLOCK_TOO_BIG, HEADER_CHECKSUM, BLOCK_CHECKSUM, CONTENT_CHECKSUM, CONTENT_LENGTH = 17, 18, 24, 25, 26, 27, 30


@pytest.fixture(scope="module")
def census():
    out = {}
    for key in D.KEYS:
        cs = D.cases(key)
        out[key] = (cs, [D.verdict(data, cap) for _, data, cap, _ in cs])
    return out


@pytest.mark.parametrize("key", D.KEYS)
def test_every_verdict_occurs(census, key):
    b = D.base(key)
    cs, vs = census[key]
    codes = collections.Counter(v.code for v in vs)
    assert any(v.code == 0 and v.prefix and v.out_len == D.CONTENT_LEN for v in vs)
    assert any(v.code == 0 and (not v.prefix or v.out_len < D.CONTENT_LEN) for v in vs)
    inner = {v.detail[2] for v in vs if v.code == DECOMPRESSION}
    assert len(inner) >= 3 and OUTPUT_TOO_SMALL in inner
    for code in (IO, BLOCK_TOO_BIG, HEADER_CHECKSUM):
        assert codes[code] > 0, code
    if b.block_checksums:
        assert codes[BLOCK_CHECKSUM] > 0
    if b.sized:
        assert codes[CONTENT_CHECKSUM] > 0 and codes[CONTENT_LENGTH] > 0
    assert collections.Counter(D.family(name) for name, _, _, _ in cs).keys() == set(D.FAMILIES)
    for (name, data, cap, k), v in zip(cs, vs):
        assert len(data) <= len(b.frame) + 80, name
        assert 0 <= k <= b.blocks


def test_the_rare_codes_occur_somewhere(census):
    codes = collections.Counter(v.code for _, vs in census.values() for v in vs)
    for code in (19, 20, 21, 22, 28, 29, 31):
        assert codes[code] > 0, code


@pytest.mark.parametrize("key", D.KEYS)
def test_the_list_is_the_same_on_every_call(key):
    assert D.cases(key) == D.cases(key)


@pytest.mark.parametrize("key", D.KEYS)
def test_the_named_deviations_are_few(census, key):
    """the rules under which lz4flex_frame_index_create may answer otherwise than the oracle: cuts the reader would wait on, and the one
    repaired header that reads as Linked -- together fewer than 5 % of the cases"""
    cs, vs = census[key]
    waits = [name for (name, _, _, _), v in zip(cs, vs) if D.reader_waits(name, v)]
    linked = [name for (name, data, _, _), v in zip(cs, vs) if D.reads_as_linked(name, data, v)]
    assert waits and all(D.family(name) == "cut" for name in waits)
    if key.startswith("ind"):                                # (only Independent base frames are given to create)
        assert linked == ["header flg bit 5"]
    else:
        linked = []
    assert len(waits) + len(linked) < 0.05 * len(cs), (len(waits), len(linked), len(cs))


@pytest.mark.parametrize("key", D.KEYS)
def test_delivered_and_twin(census, key):
    """the two helpers the GPU tests lean on: delivered() is the output where the oracle succeeds and, of a frame that was only cut, the
    content in front of the block that holds the first missing byte; checksum_twin() of a frame whose only defect is a checksum has no
    checksum error left"""
    b = D.base(key)
    cs, vs = census[key]
    for (name, data, cap, k), v in list(zip(cs, vs))[::7]:
        got = D.delivered(data, cap)
        if v.code == 0:
            assert got == v.output(), name
        elif D.family(name) == "cut":
            assert got == D.content()[:len(got)] and len(got) <= b.content_off[k], name
        if v.code in (BLOCK_CHECKSUM, CONTENT_CHECKSUM) and D.family(name) == "flip":
            t = D.verdict(D.checksum_twin(data), cap)
            assert t.code not in (BLOCK_CHECKSUM, CONTENT_CHECKSUM), name
