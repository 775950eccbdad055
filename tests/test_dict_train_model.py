"""CPU tests of the dictionary trainer's definition (tests/sim/dict_train_model.c, what lz4flex_dict_train equals byte for byte): the
known answers of the rule's edges, invariants over data kinds x sample lengths x capacities x segments, a second restatement of the rule
in numpy that must give the same bytes, and the quality condition -- a trained dictionary beats a piece of the samples on records it has
not seen, by the oracle's sizes."""
import numpy as np
import pytest

import dict_cases as D
import dict_train_model as M
import oracle_api as O

LENS = [0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 4096]
CAPS = [1, 7, 8, 63, 64, 65, 700, 32768, 65536]
SEGMENTS = [64, 512, 2048]


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


# ---- a dozen lines of numpy that say the same thing another way -----------------------------------------------------------------
def restated(samples, cap, k):
    """the rule once more: hashes by vector arithmetic, the counts by np.add.at, first(p) from the LAST earlier occurrence of p's hash,
    the scores from cumulative sums per sample"""
    hs = []
    for s in samples:
        a = np.frombuffer(bytes(s), np.uint8).astype(np.uint64)
        c = max(0, len(a) - 7)
        v = np.zeros(c, np.uint64)
        for b in range(8):
            v |= a[b:b + c] << np.uint64(8 * b)
        hs.append(((v * np.uint64(0x9E3779B185EBCA87)) >> np.uint64(44)).astype(np.int64))
    start = np.cumsum([0] + [len(h) for h in hs])
    total = int(start[-1])
    if total == 0 or cap == 0:
        return b""
    freq = np.zeros(1 << 20, np.int64)
    np.add.at(freq, np.concatenate(hs), 1)
    firsts = []
    for h in hs:
        f, last = np.ones(len(h), bool), {}
        for p, x in enumerate(h.tolist()):
            f[p] = p - last.get(x, -k) >= k
            last[x] = p
        firsts.append(f)
    nseg = -(-cap // k)
    E = max(1, min(nseg, total // (4 * k)))
    R = -(-total // E)
    remaining, idle, chosen = cap, 0, []
    for t in range(2 * nseg):
        if remaining == 0 or idle >= E:
            break
        lo, hi = (t % E) * R, min((t % E) * R + R, total)
        best, where = 0, None
        for i, h in enumerate(hs):
            if len(h) == 0 or start[i + 1] <= lo or start[i] >= hi:
                continue
            cs = np.concatenate([[0], np.cumsum(np.where(firsts[i], np.minimum(freq[h], (1 << 20) - 1), 0))])
            s = np.arange(max(lo - start[i], 0), min(hi, start[i + 1]) - start[i])
            score = cs[np.minimum(s + k - 7, len(h))] - cs[s]
            j = int(np.argmax(score))                      # (the first of equal maxima)
            if score[j] > best:
                best, where = int(score[j]), (i, int(s[j]))
        if where is None:
            idle += 1
            continue
        idle = 0
        i, s = where
        freq[hs[i][s:min(s + k - 7, len(hs[i]))]] = 0
        chosen.append(bytes(samples[i][s:s + k])[:remaining])
        remaining -= len(chosen[-1])
    return b"".join(reversed(chosen))


# ---- known answers ---------------------------------------------------------------------------------------------------------------
def test_known_answers():
    A, B = rnd(512, 1), rnd(512, 2)
    text = D.stream("text", 300, 0)
    assert M.train([A, B, A, B], 32768, 512) == (B + A, 0)                # equal scores: the lowest number first, and first means last
    assert M.train([A, B, A, B], 700, 512) == (B[:188] + A, 0)            # the second choice is clipped to its head and lands in front
    assert M.train([text] * 5, 32768, 512) == (text, 0)                   # repeated samples: once
    assert M.train([text], 100, 512) == (text[:100], 0)
    assert M.train([b"abc", b"", b"1234567"], 32768, 512) == (b"", 0)     # no sample has 8 bytes
    assert M.train([b"12345678"], 32768, 512) == (b"12345678", 0)
    assert M.train([bytes(4096)] * 4, 32768, 512) == (bytes(512), 0)
    assert M.train([], 32768, 512) == (b"", 0) and M.train([A], 0, 512) == (b"", 0)
    assert M.train([A, B, A, B], 32768, 0) == (B + A, 0)                  # segment 0 is 512


def test_too_many_candidates_is_unsupported():
    """2^32 candidates or more: the status, an empty dictionary, and no sample byte is read (the lengths alone decide)"""
    buf, offs = np.zeros(16, np.uint8), np.zeros(2, np.uint64)
    assert M.train_batch(buf, offs, np.array([0xFFFFFFFF, 0xFFFFFFFF], np.uint32)) == (b"", M.E_UNSUPPORTED)
    assert M.train_batch(buf, offs, np.array([0x80000007, 0x80000007], np.uint32)) == (b"", M.E_UNSUPPORTED)    # exactly 2^32


# ---- invariants ------------------------------------------------------------------------------------------------------------------
def batch_of(kind, length):
    """six samples of `length` bytes of a data kind"""
    flat = D.stream(kind, 6 * length, 0)
    return [flat[j * length:(j + 1) * length] for j in range(6)]


@pytest.mark.parametrize("kind", D.KINDS)
def test_invariants(kind):
    for length in LENS:
        samples = batch_of(kind, length)
        buf, offs, lens = M.pack(samples)
        moved = M.pack(samples[::-1], gap=3, lead=5)       # the same batch at other offsets: descending, odd, with gaps
        moved = (moved[0], moved[1][::-1].copy(), moved[2][::-1].copy())
        for cap in CAPS:
            for k in SEGMENTS:
                what = (kind, length, cap, k)
                d, st, picks = M.train_batch(buf, offs, lens, cap, k, with_picks=True)
                nseg = -(-cap // k)
                assert st == 0 and len(d) <= cap, what
                assert len(picks) <= 2 * nseg, what
                parts = []
                for i, s, take in picks:
                    assert 0 < take <= k and s + take <= len(samples[i]), what
                    parts.append(samples[i][s:s + take])
                assert d == b"".join(reversed(parts)), what
                if length < 8:
                    assert d == b"", what
                else:
                    assert len(d) >= min(cap, length, k), what          # something scores above 0: a whole first segment, or all the capacity
                assert M.train_batch(buf, offs, lens, cap, k) == (d, 0), what
                assert M.train_batch(*moved, cap, k) == (d, 0), what


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def small_cases():
    A, B = rnd(512, 1), rnd(512, 2)
    text = D.stream("text", 300, 0)
    yield "tie", [A, B, A, B]
    yield "five", [text] * 5
    yield "short", [b"abc", b"", b"1234567", b"12345678"]
    yield "zeros", [bytes(4096)] * 4
    for kind in D.KINDS:
        flat = D.stream(kind, 60000, 0)
        yield kind + " 300", [flat[j * 300:(j + 1) * 300] for j in range(150)]
        yield kind + " mixed", [flat[:20000], flat[20000:20005], flat[20005:24000], b"", flat[24000:60000]]


def test_a_second_restatement_gives_the_same_bytes():
    for name, samples in small_cases():
        assert sum(len(s) for s in samples) <= 65536
        for cap, k in ((32768, 512), (700, 512), (65536, 64), (5000, 2048), (1000, 100), (8192, 256)):
            assert M.train(samples, cap, k) == (restated(samples, cap, k), 0), (name, cap, k)


# ---- quality ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus():
    samples = []
    for kind, m in (("log", 512), ("json", 256), ("text", 256)):
        flat = D.stream(kind, 4096 * m, 0)
        samples += [flat[j * 4096:(j + 1) * 4096] for j in range(m)]
    unseen = [D.block(kind, 4096, salt) for kind in ("log", "json", "text") for salt in range(32)]
    return samples, unseen


def test_a_trained_dictionary_beats_a_piece_of_the_samples(corpus):
    """1 024 records of 4 KiB (log, JSON, text), 96 records that are not among them, the reference encoder's bytes.  Measured with this
    model: see the printed ratios (the prototype of the rule: none 0.478, first 32 KiB 0.452, trained 0.364)."""
    samples, unseen = corpus
    trained, st = M.train(samples, 32768, 512)
    assert st == 0 and len(trained) == 32768
    piece = b"".join(samples)[:32768]
    raw = sum(len(b) for b in unseen)
    none = sum(len(O.compress(b)) for b in unseen)
    with_piece = sum(len(O.compress_with_dict(b, piece)) for b in unseen)
    with_trained = sum(len(O.compress_with_dict(b, trained)) for b in unseen)
    print("compressed / raw: none %.3f, first 32 KiB %.3f, trained %.3f" % (none / raw, with_piece / raw, with_trained / raw))
    assert with_trained < with_piece
    assert with_trained <= 0.85 * none
    assert abs(with_trained / raw - 0.364) < 0.02       # far from the prototype's figure: the model does not implement the rule
