"""The blocks the fit tests share (tests/test_fit_model.py on the CPU, tests/test_gpu_fit.py on the GPU): written sequence by sequence with
tests/lz4_writer.py so that they sit on the edges of lz4_fit.hip -- a lane's literal and match limits, the 64-sequence chunk, the
3 840-byte tile, a sequence the whole wavefront takes.  Test infrastructure (a plain module, not a fixture)."""
import random

from lz4_writer import Writer

LITS = (0, 14, 15, 16, 269, 270, 271)
MATCHES = (4, 5, 6, 7, 8, 18, 19, 20, 273, 274)


def _offset(w, rnd, lit):
    return rnd.randint(1, min(len(w.out) + lit, 65535))


def lit_block(l, seed):
    """a leading sequence, then one sequence of l literals for every match length of MATCHES"""
    w, rnd = Writer(seed=seed), random.Random(seed)
    w.seq(3, 2, 9)
    for m in MATCHES:
        w.seq(l, _offset(w, rnd, l), m)
    return w.end(7)


def grid_block(seed=41):
    """every (l, m) of LITS x MATCHES: 71 sequences, more than one chunk"""
    w, rnd = Writer(seed=seed), random.Random(seed)
    w.seq(1, 1, 4)
    for m in MATCHES:
        for l in LITS:
            w.seq(l, _offset(w, rnd, l), m)
    return w.end(5)


def count_block(sequences, seed):
    """`sequences` sequences in all (the last one, literals only, included): 63 / 64 / 65 sit on the chunk's edge"""
    w, rnd = Writer(seed=seed), random.Random(seed)
    for j in range(sequences - 1):
        l = 1 + j % 3
        w.seq(l, _offset(w, rnd, l), 4 + (j * 5) % 9)
    return w.end(6)


def tile_edge_block(token_at, seed):
    """a block with a token at compressed offset token_at exactly (3 839: a tile's last byte, 3 840: the next tile's first), and a few
    sequences behind it"""
    w, rnd = Writer(seed=seed), random.Random(seed)
    while token_at - len(w.comp) > 24:
        w.seq(5, _offset(w, rnd, 5), 8)                      # 8 compressed bytes each
    gap = token_at - len(w.comp)                             # 9 .. 24: two sequences of 1 + l + 2 bytes
    a = (gap - 6) // 2
    w.seq(a, _offset(w, rnd, a) if len(w.out) + a else 1, 6)
    w.seq(gap - 6 - a, _offset(w, rnd, gap - 6 - a), 7)
    assert len(w.comp) == token_at
    for l, m in ((2, 9), (0, 30), (17, 5), (3, 4)):
        w.seq(l, _offset(w, rnd, l), m)
    return w.end(9)


def zero_run_block(total=300000):
    """`total` zeros: one literal, one match of total - 6 bytes, five literals -- a sequence with hundreds of length bytes"""
    w = Writer().seq(b"\0", 1, total - 6)
    return bytes(w.comp) + bytes([0x50]) + bytes(5), bytes(w.out) + bytes(5)      # (Writer.end writes random literals)


def literal_block(n=1000, seed=9):
    return Writer(seed=seed).end(n)


def shapes():
    """[(name, block, plain)]"""
    out = [("lit%d" % l, *lit_block(l, 100 + l)) for l in LITS]
    out.append(("grid", *grid_block()))
    out += [("count%d" % k, *count_block(k, 200 + k)) for k in (63, 64, 65)]
    out += [("token_at_%d" % at, *tile_edge_block(at, 300 + at)) for at in (3839, 3840)]
    out.append(("zero_run", *zero_run_block()))
    out.append(("all_literal", *literal_block()))
    return out


def shape_caps(block):
    return sorted({0, 1, 5, 6, 7, 12, 13, len(block) - 1, len(block), len(block) + 1})


def small_blocks():
    """three small blocks for every cap from 0 to 300"""
    rnd = random.Random(7)
    out = []
    for seed, (lits, matches) in enumerate((((1, 3, 0, 14, 15, 2), (4, 5, 12, 19, 6)), ((20, 0, 0, 7, 16), (40, 4, 8, 5)),
                                            ((2, 1, 30, 4, 0, 9, 3), (7, 18, 4, 20, 5, 33, 6)))):
        w = Writer(seed=500 + seed)
        for l, m in zip(lits, matches):
            l = max(l, 1) if not w.out else l
            w.seq(l, _offset(w, rnd, l), m)
        out.append(("small%d" % seed, *w.end(5 + seed * 4)))
    return out


def random_block(rnd, seed):
    """a block of 1 .. 9 sequences of random shapes (the model's cross-check with its brute force)"""
    w = Writer(seed=seed)
    for j in range(rnd.randint(0, 8)):
        l = rnd.choice([0, 1, 3, 14, 15, 16, 30, rnd.randint(0, 40)])
        if j == 0:
            l = max(l, 1)
        m = rnd.choice([4, 5, 6, 7, 8, 12, 18, 19, 20, 40, rnd.randint(4, 300)])
        w.seq(l, _offset(w, rnd, l), m)
    return w.end(rnd.choice([5, 6, 12, 20]) if w.out else rnd.choice([0, 1, 5, 20]))


# ---- damaged blocks: (name, block, promised plain, the damaged sequence's token offset, the reference's error) -----------------------
def damaged():
    import fit_model as F
    out = []
    blk, plain = count_block(40, 77)
    seqs = list(F.sequences(blk, len(blk)))
    c, p, l, m, d = seqs[20]
    at = c + 1 + F.ext(l) + l                                 # the offset of sequence 20
    bad = bytearray(blk)
    bad[at] = bad[at + 1] = 0
    out.append(("offset_zero", bytes(bad), plain, c, F.E_OFFSET_ZERO))
    # the final literal run loses its last three bytes: its token promises more than the block holds
    out.append(("truncated_literals", blk[:-3], plain, seqs[-1][0], F.E_LITERAL_OUT_OF_BOUNDS))
    # a block compressed against a dictionary: sequence 12's match starts in the 200 bytes in front of the block's own output.  The fit
    # entries take no history, so that offset is out of bounds for them as it is for a decoder without the dictionary
    w, rnd = Writer(seed=78, prefix=bytes(random.Random(78).getrandbits(8) for _ in range(200))), random.Random(78)
    for j in range(24):
        own = len(w.out) - w.base
        l = 2 + j % 4
        if j == 12:
            at = len(w.comp)
        w.seq(l, own + l + 150 if j == 12 else rnd.randint(1, own + l), 5 + j % 7)
    blk, plain = w.end(8)
    out.append(("dictionary_block", blk, plain, at, F.E_OFFSET_OUT_OF_BOUNDS))
    return out
