#!/usr/bin/env python3
"""CPU model of how often a copier wavefront of the split decoder leaves its hot loop (lz4_decompress_split.hip, Copier::run() ->
service()), for a rule that says WHICH groups write back at a visit.  No GPU, no parser, no queue: every group always has a piece.

    python tools/split_visits_model.py [--waves 100] [--seed 1] [--below 712,1080,all]

Inputs: the sequences of tests/golden/compression_66k_JSON.lz4blk (nothing else is read), cut into pieces as fe_step() cuts them
(<= 64 bytes; a match piece ends at its offset, in whole 16-byte words from 16 on).  A wavefront is 16 groups in lockstep, each
decoding 65 536 output bytes from a random sequence on (the fixture wraps around).  Per group the buffer of LayoutBig: space =
L0 + 1 952 - op; once per four steps a group with space < 4 x 64 + 64 = 320 stops and asks for a visit (iteration_begin()), as does
a record with an offset below 4 (R_RARE; the periodic path also writes back for itself below 64 bytes of space); the wavefront
finishes the four steps, then every group with a complete 16-byte unit and space < BELOW writes back (F = op & ~15) and slides (L0 = F -
512).  BELOW = 712 is the rule up to round 26 (Layout::FLUSH_AT), `all` the one since round 27.

Printed per rule: visits per wavefront, group write-backs per wavefront, wave steps, and the mean / maximum bytes written back by the
fullest group of a visit (what sets the trip count of wave_flush_slide())."""
import argparse
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_CAP, OUT_SLACK, OUT_H, PIECE, NS, BLOCK = 1984, 32, 512, 64, 4, 65536


def sequences(blk):
    """[(literal length, offset, match length)] of a raw LZ4 block (the last sequence has offset 0)"""
    out, i = [], 0
    while i < len(blk):
        tok = blk[i]
        i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                lit += blk[i]
                i += 1
                if blk[i - 1] != 255:
                    break
        i += lit
        if i >= len(blk):
            out.append((lit, 0, 0))
            break
        off = blk[i] | blk[i + 1] << 8
        i += 2
        ml = (tok & 15) + 4
        if ml == 19:
            while True:
                ml += blk[i]
                i += 1
                if blk[i - 1] != 255:
                    break
        out.append((lit, off, ml))
    return out


def pieces(seqs):
    """per sequence: ([piece lengths], rare) -- rare: the match runs in service() (offset < 4)"""
    out = []
    for lit, off, ml in seqs:
        if off == 0:            # the fixture's last literals: a group that wraps around takes them as ordinary literals
            ml = 0
        p = [PIECE] * (lit // PIECE) + ([lit % PIECE] if lit % PIECE else [])
        rare = 0 < off < 4
        if not rare and ml:
            pm = PIECE if off >= PIECE else (off & ~15 if off >= 16 else off)
            p += [pm] * (ml // pm) + ([ml % pm] if ml % pm else [])
        out.append((p, ml if rare else 0))
    return out


class Group:
    def __init__(self, seqs, start):
        self.seqs, self.si, self.pi = seqs, start, 0
        self.op = self.L0 = self.F = 0
        self.blocked = self.done = False
        self.rare = 0

    def space(self):
        return self.L0 + OUT_CAP - OUT_SLACK - self.op

    def step(self):
        if self.blocked or self.done:
            return
        p, rare = self.seqs[self.si % len(self.seqs)]
        if self.pi < len(p):
            self.op += p[self.pi]
            self.pi += 1
        if self.pi >= len(p):
            self.si, self.pi = self.si + 1, 0
            if rare:
                self.blocked, self.rare = True, rare

    def flush(self):
        self.F = self.op & ~15
        self.L0 = max(self.L0, self.F - OUT_H)


def wave(seqs, rnd, below):
    gs = [Group(seqs, rnd.randrange(len(seqs))) for _ in range(16)]
    visits = flushes = steps = 0
    fullest = []
    while not all(g.done for g in gs):
        while True:
            for g in gs:
                if not g.done and not g.blocked and g.space() < NS * PIECE + 64:
                    g.blocked = True
            for _ in range(NS):
                for g in gs:
                    g.step()
            steps += NS
            if any(g.blocked for g in gs):
                break
        visits += 1
        wb = 0
        for g in gs:
            if g.done:
                continue
            if (g.op & ~15) > g.F and (below is None or g.space() < below):
                wb = max(wb, (g.op & ~15) - g.F)
                g.flush()
                flushes += 1
            if g.rare:                                    # generic_match(): writes back for itself when it runs out of space
                n = g.rare
                while n:
                    if g.space() < 64 and g.space() < n:
                        g.flush()
                    m = min(n, g.space())
                    g.op += m
                    n -= m
                g.rare = 0
            g.blocked = False
            if g.op >= BLOCK:
                g.done = True
        fullest.append(wb)
    return visits, flushes, steps, fullest


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--waves", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--below", default="712,1080,all")
    args = ap.parse_args()
    with open(os.path.join(ROOT, "tests", "golden", "compression_66k_JSON.lz4blk"), "rb") as f:
        seqs = sequences(f.read())
    ps = pieces(seqs)
    n_pieces = sum(len(p) for p, _ in ps)
    print("%d sequences, %d pieces, %d rare; %d wavefronts of 16 groups x %d bytes per rule" % (len(seqs), n_pieces, sum(1 for _, r in ps if r), args.waves, BLOCK))
    print("floor: %.1f visits (%d / %d usable bytes less the %d a visit is asked for at)" % (
        BLOCK / (OUT_CAP - OUT_SLACK - OUT_H - NS * PIECE - 64), BLOCK, OUT_CAP - OUT_SLACK - OUT_H, NS * PIECE + 64))
    for rule in args.below.split(","):
        below = None if rule == "all" else int(rule)
        rnd = random.Random(args.seed)
        v = f = s = 0
        full = []
        for _ in range(args.waves):
            a, b, c, d = wave(ps, rnd, below)
            v, f, s = v + a, f + b, s + c
            full += d
        print("write back below %-4s  visits per wavefront %6.1f   group write-backs %7.1f   wave steps %7.1f   fullest group of a visit: mean %4.0f, max %4d bytes" % (
            rule, v / args.waves, f / args.waves, s / args.waves, sum(full) / max(len(full), 1), max(full)))


if __name__ == "__main__":
    main()
