"""CPU test of the fit rule (tests/fit_model.py, the executable statement of include/lz4flex_amd.h's "fit batches"): whatever the model
writes decodes with the oracle's decoder to src[:used] and stays inside cap; its choice is the brute force's best; the whole input is
used exactly when the block fits; more room never gives less; errors in front of the cut are the reference's, errors behind it unseen."""
import random

import pytest

import fit_cases as K
import fit_model as F
import oracle_api as O


def check(block, plain, cap, brute=True):
    out, used, st = F.fit(block, plain, cap)
    if cap == 0 and len(block) > 0:
        assert (out, used, st) == (b"", 0, F.E_OUTPUT_TOO_SMALL)
        return used
    assert st == F.OK, (cap, st)                                          # OutputTooSmall occurs at cap 0 only
    assert len(out) <= cap
    assert O.decompress(out, max(used, 1)) == ("ok", plain[:used]), cap
    assert (used == len(plain)) == (len(block) <= cap) or len(plain) == 0, cap
    if len(block) <= cap:
        assert out == block
    if brute:
        assert F.brute_force(block, plain, cap) == (out, used, st), cap
    return used


@pytest.fixture(scope="module")
def random_blocks():
    rnd = random.Random(2024)
    return [K.random_block(rnd, seed) for seed in range(40)]


def test_model_equals_brute_force_and_decodes_at_every_cap(random_blocks):
    cuts = other_k = clipped = 0
    for block, plain in random_blocks:
        for cap in range(0, len(block) + 2):
            check(block, plain, cap)
            if 0 < cap < len(block):
                seqs = list(F.sequences(block, cap))
                best = max(F.candidates(seqs, len(plain), cap), key=lambda t: t[:4])
                cuts += 1
                other_k += best[4] != len(seqs) - 1
                clipped += best[3] == F.CLIPPED
    # (the maximum over every k matters, and so does the Clipped form: the blocks exercise both)
    assert cuts > 2000 and other_k > cuts // 50 and clipped > cuts // 50, (cuts, other_k, clipped)


def test_small_blocks_at_every_cap_up_to_300():
    for name, block, plain in K.small_blocks():
        for cap in range(0, 301):
            check(block, plain, cap)


@pytest.mark.parametrize("name,block,plain", K.shapes(), ids=[s[0] for s in K.shapes()])
def test_edge_shapes_at_their_caps(name, block, plain):
    for cap in K.shape_caps(block):
        check(block, plain, cap, brute=len(plain) < 4000)


def test_used_is_monotone_in_cap():
    for name, block, plain in K.shapes() + K.small_blocks():
        last = -1
        for cap in range(0, len(block) + 17, 16):
            _out, used, st = F.fit(block, plain, cap)
            assert used >= last, (name, cap)
            last = used
        assert last == len(plain)


def test_closed_forms():
    for r in range(1, 1200):
        for avail in (0, 1, 14, 15, 16, 269, 270, 271, 5000):
            want = max(L for L in range(0, avail + 1) if F.tail(L) <= r)
            assert F.lfit(r, avail) == want, (r, avail)
    assert [F.ext(x) for x in (0, 14, 15, 269, 270, 524, 525)] == [0, 0, 1, 1, 2, 2, 3]


def test_zero_run_is_cut_by_clipping_its_match():
    block, plain = K.zero_run_block()
    out, used, st = F.fit(block, plain, 64)
    assert st == F.OK and len(out) <= 64 and used > 10000           # (a Plain cut could keep a handful of literals only)
    assert O.decompress(out, used) == ("ok", plain[:used])


def test_errors_in_front_of_the_cut_are_the_references_and_behind_it_unseen():
    for name, block, plain, at, code in K.damaged():
        names = {v: k for k, v in O.ERR_NAMES.items()}
        assert names[O.decompress(block, len(plain) + 64)[0]] == code, name       # the damage is what it is meant to be
        for cap in range(at + 1, len(block)):
            assert F.fit(block, plain, cap) == (b"", 0, code), (name, cap)
        for cap in range(1, at + 1):
            out, used, st = F.fit(block, plain, cap)
            assert st == F.OK and O.decompress(out, max(used, 1)) == ("ok", plain[:used]), (name, cap)
        assert F.fit(block, plain, len(block)) == (block, len(plain), F.OK), name  # a block that fits is not looked at


def test_a_wrong_source_length_still_gives_a_valid_block():
    block, plain = K.count_block(20, 5)
    for n in (0, 1, 7, len(plain) // 2):
        for cap in (1, 6, 20, len(block) - 1):
            out, used, st = F.fit(block, plain[:n], cap)
            assert st == F.OK and len(out) <= cap and used <= n
            assert O.decompress(out, len(plain) + 16)[0] == "ok"
