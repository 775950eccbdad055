"""Blocks WRITTEN sequence by sequence to sit on the geometry of the one-block-per-wavefront kernels (lz4_seq_walk.h: tiles of 3 840
compressed bytes in 64 parts of 60; lz4_decompress_seq.hip: a lane's literal runs and matches, chunks, the window).  Shared by
test_gpu_seq.py (the decoder) and test_gpu_size_scan.py (the size scan walks the same tiles).  Every block with sequences is checked
against the oracle here, on construction."""
import random

import oracle_api as O
from lz4_writer import Writer


def blocks():
    rnd = random.Random(606)
    out = []

    def add(name, w, tail=5):
        c, p = w.end(tail)
        st, got = O.decompress(c, len(p))
        assert st == "ok" and got == p, name            # the writer and the oracle agree on what the block says
        out.append((name, c, p))

    # ---- a lane's limits: literal runs 63 .. 66, matches 272 .. 275 (273 = 19 + 254: one length byte), 16 / 17 / 32 / 33 / 48 / 49 bytes (the pieces)
    for lit in (0, 1, 2, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 66, 200, 214, 215, 216, 269, 270, 271, 300):
        w = Writer(lit)
        w.seq(20, 7, 9)
        for _ in range(70):
            w.seq(lit, rnd.randint(24, len(w.out)), rnd.randint(4, 30))
        add("literal runs of %d" % lit, w)
    for ml in (4, 5, 7, 8, 9, 15, 16, 17, 18, 19, 20, 31, 32, 33, 34, 47, 48, 49, 50, 63, 64, 65, 128, 272, 273, 274, 275, 528, 529, 1023, 1024, 1025, 3000):
        w = Writer(ml)
        w.seq(4000, 1000, 50)
        for _ in range(70):
            w.seq(rnd.randint(0, 3), rnd.randint(ml, min(len(w.out), 3000)), ml)       # never its own output: a lane's match
        add("matches of %d" % ml, w)
    # ---- far and near: offsets around what the window holds (1 280 .. 3 584 bytes back), far matches of 63 .. 66 bytes and longer
    for ml in (4, 15, 16, 17, 33, 49, 63, 64, 65, 66, 100, 273, 274):
        w = Writer(1000 + ml)
        w.seq(9000, 5000, 40)
        for k in range(140):
            off = rnd.choice((1100, 1279, 1280, 1281, 1296, 2000, 2303, 2304, 2305, 3500, 3583, 3584, 3585, 3600, 5000, 8000, len(w.out)))
            w.seq(rnd.randint(0, 5), max(ml, min(off, len(w.out))), ml)
        add("far / near matches of %d" % ml, w)
    # ---- matches that read their own output (the wavefront's path, periodic form): every small offset, lengths short and long
    for off in (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 255, 256, 1000, 1023, 1024, 1025, 2000):
        w = Writer(2000 + off)
        w.seq(max(off, 30), off, 4)
        for ml in (5, 17, 40, off + 1, 2 * off + 3, 300, 1023, 1024, 1025, 4000, 20000):
            w.seq(rnd.randint(0, 20), off, max(ml, 4))
            w.seq(3, rnd.randint(1, min(len(w.out), 60000)), 6)
        add("own-output matches, offset %d" % off, w)
    # ---- long literal runs (memory to memory from 1 KiB on) followed by matches into them, at their ends, across them
    for run in (1000, 1023, 1024, 1025, 2048, 3583, 3584, 3585, 5000, 70000):
        w = Writer(3000 + run)
        w.seq(run, 1, 4)
        w.seq(0, run // 2, 40).seq(0, min(run + 44, 65535), 30).seq(2, 5, 4).seq(run, min(run, 65535), 50).seq(0, 51, 4)
        add("literal runs of %d" % run, w)
    # ---- tiles and parts: sequences of 3 bytes (1 280 per tile: the token list's capacity), tokens on the last byte of a tile, sequences that jump
    # over whole parts and whole tiles (literal runs inside the compressed stream), length bytes that straddle a tile's end
    w = Writer(41)
    w.seq(40, 20, 4)
    for _ in range(6000):
        w.seq(0, rnd.randint(4, 40), 4)
    add("6 000 three-byte sequences", w)
    for shift in range(0, 64, 3):
        w = Writer(500 + shift)
        w.seq(3800 + shift, 100, 12)
        for _ in range(300):
            w.seq(rnd.choice((0, 0, 1, 2, 60, 61, 120, 250, 300)), rnd.randint(4, 3000), rnd.choice((4, 19, 20, 273, 274)))
        add("tile boundary shifted by %d" % shift, w)
    w = Writer(43)
    w.seq(10, 3, 5)
    for _ in range(40):
        w.seq(rnd.choice((3839, 3840, 3841, 7680, 8000)), rnd.randint(16, 2000), rnd.randint(4, 40))
    add("literal runs that jump over tiles", w)
    # ---- chunks: 64 sequences of many bytes each (the 1 120-byte budget cuts), dense dependencies (every match reads the one before it)
    w = Writer(44)
    w.seq(600, 300, 100)
    for _ in range(500):
        w.seq(rnd.randint(0, 2), rnd.choice((100, 101, 150, 273)), rnd.choice((100, 150, 273)))
    add("long matches: chunks cut by bytes", w)
    w = Writer(45)
    w.seq(64, 30, 8)
    for _ in range(4000):
        ml = rnd.randint(4, 24)
        w.seq(rnd.choice((0, 0, 0, 1)), rnd.randint(ml, ml + 30), ml)                 # the source ends within ~ 30 bytes of the destination
    add("chains: every match reads its neighbours' output", w)
    # ---- the block's end: last literals of 0 .. 70 bytes (a lane's or the wavefront's), a block that is one literal run
    for tail in (0, 1, 5, 14, 15, 16, 63, 64, 65, 70, 300):
        w = Writer(600 + tail)
        w.seq(30, 9, 14).seq(1, 20, 5)
        add("last literals %d" % tail, w, tail)
    for n in (0, 1, 12, 13, 64, 65, 1023, 1024, 5000):
        w = Writer(700 + n)
        c, p = w.end(n)
        out.append(("literals only %d" % n, c, p))
    return out
