"""CPU tests of the partial-decode model (tests/partial_model.py, the contract of lz4flex_decompress_batch_partial): with a target no
block reaches it is the oracle's decompress_into, a target inside a valid block gives that many of the oracle's bytes, and a target in
front of a block's first error hides the error while a target behind it reports it."""
import pytest

import corpus
import oracle_api as O
import partial_model as M
import seq_blocks
import size_model as S

CODES = {v: k for k, v in S.NAMES.items()}


def oracle(c):
    """(status, bytes) of the oracle with room for anything the block can produce"""
    st, r = O.decompress(c, 255 * len(c) + 64)
    assert st != "OutputTooSmall", "the capacity must never be the limit"
    return (0, r) if st == "ok" else (CODES[st], b"")


def edge_targets(s):
    return sorted({t for t in (0, 1, s // 2, s - 1, s, s + 1) if t >= 0})


@pytest.fixture(scope="module")
def generated():
    """every block of the two generated sets, with the oracle's verdict: [(block, (status, bytes))]"""
    blocks = [c for c, _cap in corpus.adversarial_blocks()] + [c for _name, c, _p in seq_blocks.blocks()]
    return [(c, oracle(c)) for c in blocks]


def test_an_unreachable_target_is_the_oracle(generated):
    seen = set()
    for c, want in generated:
        assert M.partial(c, M.FOREVER) == want, len(c)
        seen.add(want[0])
    assert seen == {0, S.LITERAL_OUT_OF_BOUNDS, S.EXPECTED_ANOTHER_BYTE, S.OFFSET_ZERO, S.OFFSET_OUT_OF_BOUNDS}, seen


def test_targets_inside_valid_blocks(generated):
    n = 0
    for c, (st, plain) in generated:
        if st == 0:
            for t in edge_targets(len(plain)):
                assert M.partial(c, t) == (0, plain[:t]), (len(c), t)
            n += 1
    assert n > 300


def test_a_target_in_front_of_the_first_error_hides_it():
    """single-byte corruptions of an encoder's block: P, where the oracle's error is raised, comes from one walk without a target
    (Profile).  Up to the output in front of the faulty sequence -- the one that holds the corrupted byte -- the bytes are the
    uncorrupted block's; up to P the status is 0; one byte further it is the oracle's error."""
    import bisect
    plain = O.fixture_plain("compression_34k")
    good = O.compress(plain)
    starts = M.sequence_starts(good)
    ips = [ip for ip, _ in starts]
    seen = {}
    # corpus.adversarial_blocks' corruptions, and the block cut behind byte k (the faulty sequence: the one that holds the last byte there
    # is -- a block cut between two sequences fails the "a match is followed by a token" check of the first): the first 25 of every error
    damaged = [(k, good[:k] + bytes([good[k] ^ 0x5A]) + good[k + 1:]) for k in range(0, len(good), 11)]
    damaged += [(k, good[:k + 1]) for k in range(0, len(good) - 1, 97)]
    for k, bad in damaged:
        st, _ = oracle(bad)
        if st == 0 or seen.get(st, 0) >= 25:
            continue
        seen[st] = seen.get(st, 0) + 1
        prof = M.Profile(bad)
        assert prof.status == st
        before, p = starts[bisect.bisect_right(ips, k) - 1][1], len(prof.out)
        assert before <= prof.before <= p and prof.out[:before] == plain[:before], k
        for t in sorted(t for t in {0, 1, before // 2, before - 1, before} if 0 <= t <= before):
            assert M.partial(bad, t) == (0, plain[:t]), (k, t)
        for t in sorted({before, before + 1, (before + p) // 2, p - 1, p} & set(range(before, p + 1))):
            got = M.partial(bad, t)
            assert got[0] == 0 and len(got[1]) == t and got == prof.at(t), (k, t)
        for t in (p + 1, p + 2, p + 1000, M.FOREVER):
            assert M.partial(bad, t) == (st, b"") == prof.at(t), (k, t)
    assert set(seen) == {S.LITERAL_OUT_OF_BOUNDS, S.EXPECTED_ANOTHER_BYTE, S.OFFSET_ZERO, S.OFFSET_OUT_OF_BOUNDS}, seen


def test_one_walk_gives_every_target(generated):
    """Profile.at (what the GPU tests compare whole sets with) is partial at every target, errors included"""
    for c, (st, plain) in generated[::7]:
        prof = M.Profile(c)
        p = len(prof.out)
        for t in sorted({0, 1, p // 2, p - 1, p, p + 1, p + 70000} - {-1}):
            assert prof.at(t) == M.partial(c, t), (len(c), t)
    assert M.partial(b"", 0) == M.Profile(b"").at(0) == (S.EXPECTED_ANOTHER_BYTE, b"")      # an empty block: before anything else
    assert M.partial(b"\x10a", 0) == (0, b"")


def test_hand_written_blocks():
    """the writer's plain text is the oracle's; every listed target gives its prefix -- also where the block ends in a match, which is
    an error for the oracle and for every target behind the match's last byte"""
    kinds = set()
    for name, c, plain, targets in M.writer_cases():
        st, got = oracle(c)
        ends_in_match = name.startswith("the block ends in a match")
        if ends_in_match:
            assert st == S.EXPECTED_ANOTHER_BYTE, name
        else:
            assert (st, got) == (0, plain), name
        for t in targets:
            want = (S.EXPECTED_ANOTHER_BYTE, b"") if ends_in_match and t > len(plain) else (0, plain[:t])
            assert M.partial(c, t) == want, (name, t)
        assert {0, 1, len(plain) - 1, len(plain), len(plain) + 1} <= set(targets), name
        kinds.add(name.split(":")[0].split(",")[0])
    assert len(kinds) > 30


def test_corrupted_hand_written_blocks():
    """the damaged place decides: in front of the stop the oracle's error, in the crossing sequence the error or the bytes depending on
    which comes first, behind the stop nothing"""
    outcomes = set()
    for name, c, targets in M.corrupted_cases():
        st, _ = oracle(c)
        assert st != 0, name
        prof = M.Profile(c)
        for t in targets:
            got = M.partial(c, t)
            assert got == prof.at(t), (name, t)
            assert got[0] in (0, st), (name, t)
            outcomes.add((name.split(",")[-1].strip(), got[0] != 0))
    for where in ("in front of the stop", "the crossing sequence", "right behind the stop", "a tile later"):
        assert (where, True) in outcomes and (where, False) in outcomes, where
