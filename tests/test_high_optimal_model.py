"""CPU: the scalar definition of compress_mode 2 ("high") under "compress_parse" 1 (tests/sim/high_optimal_model.c).  With parse 0 it is
the two existing definitions, byte for byte; with parse 1 every block decodes through the oracle to its input (with a dictionary and
behind a history too), its lengths are what a plain restatement of the rule gives from best[], and the known sizes are pinned."""
import random

import pytest

import hc_dict_model as D
import hc_linked_model as K
import hc_model as H
import hc_optimal_model as P
import oracle_api as O
from test_high_model import inputs as plain_inputs

DEPTHS = (1, 4, 16, 64)


def J():
    return O.fixture_plain("compression_66k_JSON")


def T():
    return O.fixture_plain("compression_65k")


def end_rules(comp, n):
    """src/block/mod.rs:37-61: the last 5 bytes are literals, the last match starts at or before n - 12"""
    seqs = H.walk(comp)
    pos, last_match = 0, None
    for lit, ml in seqs:
        pos += lit
        if ml:
            assert ml >= 4
            last_match = pos
            pos += ml
    assert pos == n
    if len(seqs) > 1:
        assert seqs[-1][0] >= 5 and last_match <= n - 12


@pytest.mark.parametrize("i", range(len(plain_inputs())))
def test_parse_0_is_the_plain_model_and_parse_1_round_trips(i):
    data = bytes(plain_inputs()[i])
    for depth in DEPTHS:
        assert P.compress(data, b"", depth, 0) == H.compress(data, depth), depth
        comp = P.compress(data, b"", depth, 1)
        assert len(comp) <= O.max_out(len(data))
        assert O.decompress(comp, len(data)) == ("ok", data), depth
        end_rules(comp, len(data))


def dict_cases():
    """the (block, dictionary) pairs of tests/test_high_dict_model.py: its known answers, its 24 cases, the no-dictionary lengths"""
    j, t = J(), T()
    out = [(data, d) for data in (b"", j[:11], j[:13], j[:4096], j, (j * 3)[:150000]) for d in (b"", j[:1], j[:3])]
    for s in (j, t):
        for dl in (4096, 32768, 40000):
            for blk in (slice(40000, 44096), slice(50000, 50100), slice(41000, None), slice(40000, 40013)):
                out.append((s[blk], s[:dl]))
    out.append(((j * 3)[:150000], j[100:30000]))
    rnd = random.Random(5)
    d = bytes(rnd.getrandbits(8) for _ in range(5000))
    out.append((d[-40:] * 2 + bytes(rnd.getrandbits(8) for _ in range(30)), d))
    rnd = random.Random(6)
    d = bytes(rnd.getrandbits(8) for _ in range(32768))
    out.append((bytes(rnd.getrandbits(8) for _ in range(32764)) + d[:4] + bytes(rnd.getrandbits(8) for _ in range(40)), d))
    return out


@pytest.mark.parametrize("depth", (1, 16))
def test_with_a_dictionary(depth):
    for data, d in dict_cases():
        assert P.compress(data, d, depth, 0) == D.compress(data, d, depth), (len(data), len(d))
        comp = P.compress(data, d, depth, 1)
        assert len(comp) <= O.max_out(len(data))
        assert O.decompress(comp, len(data), dict_data=d if len(d) >= 1 else None) == ("ok", data), (len(data), len(d))
        end_rules(comp, len(data))


def test_fuzz_with_a_dictionary_through_the_oracles_decoder():
    rnd = random.Random(99)
    j, t = J(), T()
    noise = bytes(rnd.getrandbits(8) for _ in range(70000))
    pool = (j * 3, t * 3, noise * 3, bytes(200000), (bytes(range(256)) * 800))
    for _ in range(150):
        dl = rnd.choice((0, 3, 4, 5, 100, 4096, 32767, 32768, 32769, 70000))
        n = rnd.choice((0, 1, 11, 12, 13, 100, 2047, 2048, 2049, 4096, 32767, 32768, 32769, 40000, 65536, 65537))
        depth = rnd.choice(DEPTHS)
        src = rnd.choice(pool)
        at = rnd.randrange(0, 1000)
        d = src[at:at + dl]
        other = rnd.choice(pool) if rnd.random() < 0.2 else src
        at2 = rnd.randrange(0, len(other) - n)
        data = other[at2:at2 + n]
        assert P.compress(data, d, depth, 0) == D.compress(data, d, depth), (dl, n, depth)
        comp = P.compress(data, d, depth, 1)
        assert O.decompress(comp, n, dict_data=d if d else None) == ("ok", data), (dl, n, depth)
        end_rules(comp, n)


def test_behind_a_history():
    """a stream cut into blocks, each behind everything in front of it: parse 0 is tests/hc_linked_model.py, parse 1 decodes"""
    stream = (J() * 2)[:150000]
    for cut in (4096, 65536, 70001):
        plain = b""
        for at in range(0, len(stream), cut):
            n = min(cut, len(stream) - at)
            assert P.block(stream, at, n, at, 16, 0) == K.block(stream, at, n, at, 16), (cut, at)
            comp = P.block(stream, at, n, at, 16, 1)
            hist = plain[-65536:]
            assert O.decompress(comp, n, dict_data=hist if hist else None) == ("ok", stream[at:at + n]), (cut, at)
            plain += stream[at:at + n]


# ---- the rule, restated: from best[] of one chunk to len'[] (the issue's loop; nothing of the model's is called)
def ext(v):
    return 0 if v < 15 else (v - 15) // 255 + 1


def restated(best_len):
    cn = len(best_len)
    cost, pick = [None] * cn, [0] * cn
    inf = float("inf")
    for j in range(cn - 1, -1, -1):
        se = min((j // 2048 + 1) * 2048, cn)
        co = lambda x: 0 if x >= se else cost[x]      # noqa: E731
        L, c, pk = best_len[j], inf, 0
        if L >= 4:
            room = se - j
            lp = min(L, room)
            c, pk = 3 + ext(0 if lp < 4 else lp - 4) + co(j + L), L
            for l in range(min(L - 1, 35, room), 3, -1):
                v = 3 + ext(l - 4) + co(j + l)
                if v < c:
                    c, pk = v, l
        if 1 + co(j + 1) < c:
            c, pk = 1 + co(j + 1), 0
        cost[j], pick[j] = c, pk
    return pick


def small_inputs():
    rnd = random.Random(23)
    j, t = J(), T()
    runs = bytearray()
    while len(runs) < 8192:
        runs += bytes([rnd.getrandbits(8)]) * rnd.randint(1, 300)
    ab = bytes(rnd.choice(b"ab") for _ in range(5000))
    out = [j[:8192], j[3000:3000 + 4097], t[:8192], t[100:100 + 2049], t[:2048], t[:2047], bytes(8192), bytes(runs[:8192]), ab, b"ab" * 3000,
           bytes(rnd.getrandbits(8) for _ in range(3000)), j[:40], j[:12], j[:11], b""]
    # matches that cross a segment's end: a 300-byte phrase repeated so that copies straddle 2 048, 4 096 and 6 144 at every phase
    phrase = bytes(rnd.getrandbits(8) for _ in range(300))
    for lead in (0, 1, 2, 3, 17, 29, 281, 297):
        out.append((bytes(rnd.getrandbits(8) for _ in range(1500 + lead)) + phrase * 20)[:8192])
    return out


@pytest.mark.parametrize("i", range(len(small_inputs())))
def test_lengths_are_the_restated_rule(i):
    data = small_inputs()[i]
    for d in (b"", J()[:5000]):
        for depth in (1, 16):
            _, best_len, best_off, pick = P.trace(data, d, depth, 1)
            assert pick == restated(best_len), (len(data), len(d), depth)
            _, lazy_len, lazy_off, lazy_pick = P.trace(data, d, depth, 0)
            assert (lazy_len, lazy_off) == (best_len, best_off) and lazy_pick == best_len


KNOWN = {       # (input, depth): (lazy, optimal)
    ("compression_34k", 4): (16926, 16541), ("compression_34k", 16): (16335, 16038), ("compression_34k", 64): (16125, 15860),
    ("compression_65k", 4): (31186, 30394), ("compression_65k", 16): (29926, 29372), ("compression_65k", 64): (29549, 29086),
    ("compression_66k_JSON", 4): (13257, 12870), ("compression_66k_JSON", 16): (12843, 12414), ("compression_66k_JSON", 64): (12390, 12052),
}


@pytest.mark.parametrize("stem,depth", sorted(KNOWN))
def test_known_sizes_of_the_fixtures(stem, depth):
    data = O.fixture_plain(stem)
    lazy, optimal = len(P.compress(data, b"", depth, 0)), len(P.compress(data, b"", depth, 1))
    print("%s depth %d: lazy %d optimal %d" % (stem, depth, lazy, optimal))
    assert (lazy, optimal) == KNOWN[(stem, depth)]
    assert optimal < lazy


@pytest.mark.parametrize("depth", (4, 16, 64))
def test_known_size_of_zeros(depth):
    z = bytes(65536)
    assert (len(P.compress(z, b"", depth, 0)), len(P.compress(z, b"", depth, 1))) == (267, 267)
    assert O.decompress(P.compress(z, b"", depth, 1), 65536) == ("ok", z)


def test_known_size_of_the_log_stream():
    from lz4_flex_amd import workloads
    log = bytes(workloads.log_stream(0, 1 << 20).numpy())
    got = {depth: (len(P.compress(log, b"", depth, 0)), len(P.compress(log, b"", depth, 1))) for depth in (4, 16, 64)}
    print(got)
    assert got == {4: (274912, 265686), 16: (259570, 251701), 64: (252256, 245220)}
