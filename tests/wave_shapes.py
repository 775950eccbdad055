"""A corpus that makes the throughput ("wave") encoder write every sequence shape, and the classifier that proves it.

The kernel (lz4_flex_amd/csrc/lz4_compress_wave.hip) writes a sequence in one of four places: lane-parallel in encode_seqs (fewer
than 270 own literals and a match of fewer than 274 bytes), whole-wavefront in emit_generic (the "hard" ones), the token and
literals of a segment's first sequence in place_segment (its carried literals `pend` plus its own), and a run window's one
sequence.  Each has its own length-byte arithmetic, so each needs sequences on both sides of every length-byte boundary.

The generator plants sequences in random bytes: for each, `lit` fresh literals, then a copy of `ml` bytes from 64 to 100 bytes
back (far enough that the source is in the hash table when the position looks it up, near enough that it is rarely evicted), with
the bytes on either side made to differ so that the match neither grows nor shrinks.  Where the plants go is decided relative to
the segments of the block, which are read from the scalar model's trace (wave_model.trace) of the same geometry.  Chance still
shifts a parse now and then, so coverage is not assumed: classes() measures it on the model's own output, and the CPU test
asserts REQUIRED for every configuration."""
import random

import wave_model as W

DMIN, DMAX = 64, 100

# encoder configurations that move segment and window starts: name -> (block length without history, compress() keywords)
CONFIGS = {
    "sub1": (65536, dict(sub=1)),
    "sub2": (65536, dict(sub=2)),
    "sub3": (65536, dict(sub=3)),
    "sub4": (65536, dict(sub=4)),
    "slide0": (3 * 65536 + 4321, dict(slide=0)),
    "slide1": (3 * 65536 + 4321, dict(slide=1)),
    "slide2": (3 * 65536 + 4321, dict(slide=2)),
    "hist": (3 * 65536 + 4321, dict(hist=W.HIST)),
}
SINGLE_WINDOW = {"sub1"}          # (the configurations whose blocks are one window: no window can be empty)

LP_LITS = (0, 14, 15, 16, 17, 31, 32, 33, 268, 269)
LP_MLS = (18, 19, 272, 273)
HARD_LITS = (270, 271, 524, 525, 526)
HARD_MLS = (274, 275, 528, 529)
FIRST_LITS = (0, 14, 15, 269, 270, 524, 525)
FINAL_LITS = (14, 15, 269, 270, 524, 525)     # (never fewer than 5: the last 5 bytes are literals)
LONG_CARRY = 16080                            # literal length bytes of a carried run: 1 + (L - 15) // 255 + 1 > 64

REQUIRED = (
    ["lane: lit %d" % v for v in LP_LITS]
    + ["lane: lit %% 16 == %d (16 <= lit < 270)" % r for r in range(16)]
    + ["lane: literal source %% 16 == %d" % r for r in range(16)]
    + ["lane: match %d" % v for v in LP_MLS]
    + ["hard: lit %d" % v for v in HARD_LITS] + ["hard: lit >= 1024"]
    + ["hard: match %d" % v for v in HARD_MLS]
    + ["hard: lane 0 of a later call", "hard: lane 63", "hard: two in one call", "hard: segment's first"]
    + ["call: 64 lanes", "call: second call of a segment"]
    + ["first: lit %d" % v for v in FIRST_LITS]
    + ["first: carried from the previous segment's tail", "first: carried across a segment without sequences",
       "first: carried across a window without sequences", "first: lit >= %d" % LONG_CARRY]
    + ["final: lit %d" % v for v in FINAL_LITS]
    + ["run: a run window"]
)


def required(config):
    if config in SINGLE_WINDOW:
        return [c for c in REQUIRED if c != "first: carried across a window without sequences"]
    return list(REQUIRED)


# ---- the classifier ------------------------------------------------------------------------------------------------------------

def classes(seqs, segs):
    """the REQUIRED classes that the trace of one block (wave_model.trace) holds"""
    got = set()
    wbase = {int(g["win"]): int(g["wbase"]) for g in segs}
    seg_list = sorted((int(g["s0"]), int(g["s1"]), int(g["win"]), int(g["wj"])) for g in segs)
    has_seq = {(int(s["win"]), int(s["wj"])) for s in seqs if s["mlen"]}
    by_call = {}
    for s in seqs:
        lit, ml, first = int(s["lit_len"]), int(s["mlen"]), bool(s["first"])
        if ml == 0:                                                   # the final literals
            if lit in FINAL_LITS:
                got.add("final: lit %d" % lit)
            continue
        if s["run"]:
            got.add("run: a run window")
            continue
        own = lit - int(s["pend"]) if first else lit                  # what encode_seqs sees: a first sequence's own literals
        hard = own >= 270 or ml >= 274
        key = (int(s["win"]), int(s["wj"]), int(s["call"]))
        by_call.setdefault(key, []).append((int(s["lane"]), hard))
        if ml in HARD_MLS:
            got.add("hard: match %d" % ml)
        if first:
            if lit in FIRST_LITS:
                got.add("first: lit %d" % lit)
            if lit >= LONG_CARRY:
                got.add("first: lit >= %d" % LONG_CARRY)
            if hard:
                got.add("hard: segment's first")
            if s["pend"]:
                a, b = int(s["lit_start"]), int(s["lit_start"]) + int(s["pend"])    # the carried literals
                for s0, s1, win, wj in seg_list:
                    if s0 <= a < s1 and (win, wj) in has_seq:
                        got.add("first: carried from the previous segment's tail")
                    if a <= s0 and s1 <= b and (win, wj) not in has_seq and win == s["win"]:
                        got.add("first: carried across a segment without sequences")
                whole = {}
                for s0, s1, win, wj in seg_list:
                    whole.setdefault(win, []).append(a <= s0 and s1 <= b)
                if any(all(v) for w, v in whole.items() if w != s["win"]):
                    got.add("first: carried across a window without sequences")
            continue
        if hard:
            if lit in HARD_LITS:
                got.add("hard: lit %d" % lit)
            if lit >= 1024:
                got.add("hard: lit >= 1024")
            if s["lane"] == 0 and s["call"] >= 1:
                got.add("hard: lane 0 of a later call")
            continue
        if lit in LP_LITS:
            got.add("lane: lit %d" % lit)
        if lit >= 16:
            got.add("lane: lit %% 16 == %d (16 <= lit < 270)" % (lit % 16))
            got.add("lane: literal source %% 16 == %d" % ((int(s["lit_start"]) - wbase[int(s["win"])]) % 16))
        if ml in LP_MLS:
            got.add("lane: match %d" % ml)
    for (win, wj, call), lanes in by_call.items():
        if call >= 1:
            got.add("call: second call of a segment")
        if len(lanes) == 64:
            got.add("call: 64 lanes")
        if sum(h for _, h in lanes) >= 2:
            got.add("hard: two in one call")
        if any(lane == 63 and h for lane, h in lanes):
            got.add("hard: lane 63")
    return got


# ---- the generator -------------------------------------------------------------------------------------------------------------

class _Block:
    def __init__(self, n, kw, seed):
        self.rnd = random.Random(seed)
        self.hist = kw.get("hist", 0)
        self.kw = kw
        self.n = self.hist + n
        self.buf = bytearray(self.rnd.getrandbits(8) for _ in range(self.n))
        _, segs = W.trace(bytes(self.buf), **kw)                     # random bytes: no matches, no run windows -- the bare geometry
        self.segs = sorted(segs.tolist(), key=lambda g: g[3])         # (win, wj, wbase, s0, s1, run)
        self.events = []                                              # (match start, match length)

    def fill(self, k, items, tail=None, span=0, close_ml=8, start=0):
        """segment k: the sequences `items` [(lit, ml), ...] from `start` bytes into it on (the first lit: its own literals), as
        many as fit; returns how many did.  tail: then one more match that ends `tail` bytes before the segment's end; span: ... that
        reaches `span` bytes into the next segment (whose first sequence is then the rest of it: no literals)"""
        _, _, wbase, s0, s1, _ = self.segs[k]
        items = list(items)
        if items and not start and s0 + items[0][0] - wbase < DMAX + 8:     # (a match needs its source inside the window)
            items[0] = (items[0][0] + DMAX + 8, items[0][1])
        if span:
            stop = s1 - 24
        elif tail is not None:
            stop = s1 - tail - close_ml - 2
        else:
            stop = s1
        p, placed = s0 + start, 0
        for lit, ml in items:
            if p + lit + ml > min(stop, self.n - 12):
                break
            self.events.append((p + lit, ml))
            p += lit + ml
            placed += 1
        if span:
            self.events.append((s1 - 16, 16 + span))
        elif tail is not None and p + close_ml <= s1 - tail:
            self.events.append((s1 - tail - close_ml, close_ml))
        return placed

    def data(self):
        buf, rnd = self.buf, self.rnd
        ev = sorted(self.events)
        prev_end, prev_d = -1, 0
        for p, ml in ev:
            assert p >= prev_end and p + ml <= self.n - 5 and p <= self.n - 12, (p, ml, prev_end)
            cands = [d for d in range(DMIN, DMAX + 1)]
            rnd.shuffle(cands)
            for d in cands:
                if p != prev_end or (d != prev_d and buf[p - d] != buf[p - prev_d]):
                    break
            if p - 1 >= prev_end:                                     # the literal in front differs from the source's: no longer match
                avoid = {buf[p - 1 - d]} | ({buf[prev_end - prev_d]} if p - 1 == prev_end else set())
                buf[p - 1] = next(v for v in range(256) if v not in avoid) if buf[p - 1] in avoid else buf[p - 1]
            for i in range(ml):
                buf[p + i] = buf[p - d + i]
            e = p + ml
            if e < self.n and buf[e] == buf[e - d]:                   # the byte behind differs: the match ends here
                buf[e] = (buf[e] + 1 + rnd.randrange(255)) % 256
            prev_end, prev_d = e, d
        return bytes(buf)


def _parade():
    """every lane-parallel and hard non-first shape, then seventeen 16-literal sequences whose sources step through every residue"""
    out = []
    mls = (4, 5, 18, 19, 6, 272, 7, 273)
    for i, lit in enumerate((0, 14, 15, 16, 17, 31, 32, 33, 268, 269) + tuple(range(18, 31))):
        out.append((lit, mls[i % len(mls)]))
    out += [(3, ml) for ml in HARD_MLS]
    out += [(lit, 5) for lit in HARD_LITS + (1030,)]
    out += [(4, ml) for ml in HARD_MLS[::-1]]
    out += [(16, 17)] * 17                                            # 33 bytes a step: the literals start at every residue mod 16
    return out


def _cluster(rnd):
    """64 sequences for one call (the last two hard), then a hard one that opens the segment's second call"""
    out = [(30, 6)]
    for _ in range(61):
        out.append((rnd.randrange(4), rnd.choice([m for m in (4, 5, 6, 7) if m != out[-1][1]])))
    out += [(2, 274), (1, 275), (300, 6)]
    return out


def _segs_fill(b, items, first=0, lead=32):
    """items over segments first, first + 1, ...: each segment opens with `lead` literals and a match"""
    k = first
    items = list(items)
    while items and k < len(b.segs) - 1:
        items = items[max(0, b.fill(k, [(lead, 6)] + items) - 1):]
        k += 1
    return k


def blocks(config, seed=0):
    """the corpus of one configuration: a list of (data, kwargs for wave_model.compress / trace); data starts with the history"""
    n, kw = CONFIGS[config]
    out = []
    rnd = random.Random(sorted(CONFIGS).index(config) * 1000 + seed)
    finals = list(FINAL_LITS)

    def done(b):
        out.append((b.data(), dict(kw)))

    def close_final(b):                                               # the last match ends `tail` bytes before the block's end
        tail = finals.pop(0) if finals else 100
        p = b.n - tail - 8
        b.events = [(q, ml) for q, ml in b.events if q + ml < p - 1]
        b.events.append((p, 8))

    for rep in range(2):
        # 1. the parade
        b = _Block(n, kw, 1000 * rep + 1)
        k = _segs_fill(b, _parade())
        if k < len(b.segs) - 1:
            close_final(b)
        done(b)
        # 2. a 64-lane call in every other segment
        b = _Block(n, kw, 1000 * rep + 2)
        for k in range(rep, len(b.segs) - 1, 2):
            b.fill(k, _cluster(rnd))
        close_final(b)
        done(b)
        # 3. segment boundaries: carried + own literals of every first sequence length class (a match across the boundary: none),
        # every seventh segment without sequences (its literals are carried on)
        b = _Block(n, kw, 1000 * rep + 3)
        splits = [("span", 6), (7, 7), (15, 0), (1, 268), (0, 270), (262, 262), (300, 225), (100, 170), (12, 3), (424, 100), (25, 500)]
        splits = splits[rep:] + splits[:rep]
        empty = lambda k: k % 7 == 5
        for k in range(len(b.segs) - 1):
            if empty(k):
                continue
            into, out_ = splits[(k - 1) % len(splits)], splits[k % len(splits)]
            if empty(k + 1) and out_[0] == "span":
                out_ = (30, 0)
            start, items = 0, [(40, 300)]
            if k > 0 and into[0] == "span" and not empty(k - 1):
                start, items = into[1], []
            elif k > 0:
                items = [(into[1], 6 if k % 3 else 300)]
            items += [(20, 7), (3, 5)]
            if out_[0] == "span":
                b.fill(k, items, span=out_[1], start=start)
            else:
                b.fill(k, items, tail=out_[0], start=start)
        close_final(b)
        done(b)
    # 4. long carries: one whole window (or three segments) without sequences between two that have some
    b = _Block(n, kw, 4)
    wins = sorted({g[0] for g in b.segs})
    if len(wins) >= 2:
        empty = wins[1] if len(wins) >= 3 else wins[0]
        ks = [k for k, g in enumerate(b.segs) if g[0] != empty]
    else:
        ks = [k for k in range(len(b.segs)) if k not in (3, 4, 5)]
    for k in ks[:-1]:
        b.fill(k, [(50, 6), (20, 9)], tail=11)
    close_final(b)
    done(b)
    # 5. a run window (index_window: one sequence, emit_generic) between windows with sequences; sub-windows all start at the
    # block's start, so there the block's first sub-window is the run
    b = _Block(n, kw, 5)
    wins = sorted({g[0] for g in b.segs})
    w0 = wins[1] if "sub" not in kw and len(wins) >= 3 else wins[0]
    lo = min(g[2] for g in b.segs if g[0] == w0)
    hi = max(g[4] for g in b.segs if g[0] == w0)
    b.buf[lo:hi] = bytes(hi - lo)
    for k, g in enumerate(b.segs[:-1]):
        if g[4] + 2 * DMAX < lo or g[3] > hi + 2 * DMAX:
            b.fill(k, [(50, 6), (20, 9)], tail=11)
    if hi < b.n - 600:
        close_final(b)
    done(b)
    # 6. the remaining final-literal lengths
    while finals:
        b = _Block(n, kw, 100 + len(finals))
        _segs_fill(b, [(5, 8)] * 10, first=len(b.segs) // 2)
        close_final(b)
        done(b)
    return out


def coverage(config):
    got = set()
    for data, kw in blocks(config):
        got |= classes(*W.trace(data, **kw))
    return got
