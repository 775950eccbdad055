"""CPU tests of the model of partial decode against a dictionary (tests/partial_dict_model.py, the contract of
lz4flex_decompress_batch_partial_shared_dict / _dict_set): the writer's blocks say what the oracle says with the same dictionary, the
model at every target gives that many of the oracle's bytes, a damaged block's error is the oracle's, one walk gives every target, and
without a dictionary the model is tests/partial_model.py."""
import pytest

import oracle_api as O
import partial_dict_model as D
import partial_model as M
import size_model as S

CODES = {v: k for k, v in S.NAMES.items()}


def oracle(c, dic, room):
    st, r = O.decompress(c, room, dict_data=dic)
    assert st != "OutputTooSmall", "the capacity must never be the limit"
    return (0, r) if st == "ok" else (CODES[st], b"")


@pytest.fixture(scope="module", params=D.DICT_LENGTHS)
def dic(request):
    return D.dictionary(request.param)


def test_valid_cases_are_the_oracles_prefixes(dic):
    """the writer's plain text is the oracle's with this dictionary; every listed target gives its prefix -- also where the block ends
    in a match, which is an error for the oracle and for every target behind the match's last byte"""
    cases = D.dict_cases(dic)
    kinds = set()
    for name, c, plain, targets in cases:
        st, got = oracle(c, dic, len(plain) + 64)
        ends_in_match = name.startswith("the block ends in")
        if ends_in_match:
            assert st == S.EXPECTED_ANOTHER_BYTE, name
        else:
            assert (st, got) == (0, plain), name
        prof = D.Profile(c, dic)
        assert {0, 1, len(plain) - 1, len(plain), len(plain) + 1} <= set(targets), name
        for t in targets:
            want = (S.EXPECTED_ANOTHER_BYTE, b"") if ends_in_match and t > len(plain) else (0, plain[:t])
            assert D.partial_with_dict(c, t, dic) == want == prof.at(t), (name, t)
        kinds.add(name.split(":")[0])
    assert {"first sequence", "straddling", "a long run"} <= kinds and any(k.startswith("the block ends in") for k in kinds)
    if len(dic) >= 10:
        assert "far" in kinds
    # the blocks do reach into the dictionary: without it every one of them is an error at its full size
    assert all(M.partial(c, M.FOREVER)[0] == S.OFFSET_OUT_OF_BOUNDS for _n, c, _p, _t in cases)


def test_damaged_cases(dic):
    """with a target no block reaches the model gives the oracle's error; the damaged place decides what a target sees; one walk gives
    every target.  An offset one past the dictionary exists only below 65 535 bytes of dictionary: from there on the model calls no
    offset out of bounds"""
    outcomes, kinds = set(), set()
    for name, c, targets in D.damaged_cases(dic):
        st, _ = oracle(c, dic, 255 * len(c) + 64)
        assert st != 0, name
        assert D.partial_with_dict(c, M.FOREVER, dic) == (st, b""), name
        prof = D.Profile(c, dic)
        for t in targets:
            got = D.partial_with_dict(c, t, dic)
            assert got == prof.at(t), (name, t)
            assert got[0] in (0, st), (name, t)
            outcomes.add((name.split(",")[-1].strip(), got[0] != 0))
        kinds.add(st)
    for where in ("in front of the stop", "the crossing sequence", "right behind the stop", "a tile later"):
        assert (where, True) in outcomes and (where, False) in outcomes, where
    if len(dic) < 65535:
        assert kinds == {S.OFFSET_ZERO, S.OFFSET_OUT_OF_BOUNDS}
    else:
        assert kinds == {S.OFFSET_ZERO}
        from lz4_writer import Writer
        for off in (1, 4096, 65534, 65535):
            w = Writer(3, prefix=dic[-D.WINDOW:])
            w.bad_seq(0, off, 8)
            c = w.end(5)[0]
            assert D.partial_with_dict(c, M.FOREVER, dic)[0] == 0 == oracle(c, dic, 4096)[0], off


def test_the_untruncated_length_is_checked():
    """70 001 bytes of dictionary, of which 65 536 are read: offset 65 535 at op = 0 is fine; with the same last 64 KiB and a length of
    65 534 it is one too many"""
    from lz4_writer import Writer
    long = D.dictionary(70001)
    w = Writer(4, prefix=long[-D.WINDOW:])
    w.seq(0, 65535, 8)
    c, plain = w.end(5)
    assert D.partial_with_dict(c, M.FOREVER, long) == (0, plain) == oracle(c, long, 4096)
    short = long[-65534:]
    assert D.partial_with_dict(c, M.FOREVER, short) == (S.OFFSET_OUT_OF_BOUNDS, b"") == oracle(c, short, 4096)
    assert D.partial_with_dict(c, 0, short) == (0, b"")


def test_without_a_dictionary_it_is_the_plain_model():
    for name, c, _plain, targets in M.writer_cases():
        for t in targets:
            assert D.partial_with_dict(c, t, b"") == M.partial(c, t), (name, t)
    for name, c, targets in M.corrupted_cases():
        for t in targets:
            assert D.partial_with_dict(c, t, b"") == M.partial(c, t) == D.Profile(c, b"").at(t), (name, t)
    assert D.partial_with_dict(b"", 0, b"abc") == D.Profile(b"", b"abc").at(0) == (S.EXPECTED_ANOTHER_BYTE, b"")
    assert D.partial_with_dict(b"\x10a", 0, b"abc") == (0, b"")


def test_plain_cases_against_a_dictionary():
    """partial_model's hand-written sets against a dictionary they never reach into: the plain results, except that an offset one past
    the output now lies in the dictionary"""
    for n in (17, 70001):
        dic = D.dictionary(n)
        for name, c, _plain, targets in M.writer_cases():
            for t in targets:
                assert D.partial_with_dict(c, t, dic) == M.partial(c, t), (name, t)
        differ = set()
        for name, c, targets in M.corrupted_cases():
            prof = D.Profile(c, dic)
            for t in targets:
                got = D.partial_with_dict(c, t, dic)
                assert got == prof.at(t), (name, t)
                if got != M.partial(c, t):
                    assert name.startswith("an offset one past the output") and M.partial(c, t)[0] == S.OFFSET_OUT_OF_BOUNDS, (name, t)
                    differ.add(name)
        assert len(differ) == 4, differ
