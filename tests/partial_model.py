"""A pure-Python model of lz4flex_decompress_batch_partial (include/lz4flex_amd.h, "PARTIAL DECODE"): src/block/decompress.rs:201-449
decoded until `target` bytes exist.  tests/test_partial_model.py pins it to the oracle; the GPU tests (tests/test_gpu_partial.py) check
the kernels against it.  Built on the walk of tests/size_model.py, with the bytes."""
from size_model import EXPECTED_ANOTHER_BYTE, LITERAL_OUT_OF_BOUNDS, NAMES, OFFSET_OUT_OF_BOUNDS, OFFSET_ZERO, OK

FOREVER = 1 << 31     # a target no block of the test sets reaches


def _run(b, target):
    """the contract, line by line: (status, the output so far, its bytes in front of the sequence the walk ended in)"""
    n = len(b)
    if n == 0:
        return EXPECTED_ANOTHER_BYTE, bytearray(), 0        # :207-209, before anything else
    out = bytearray()
    ip = op = before = 0                                    # (op == len(out))
    while op < target:
        before = op
        token = b[ip]
        ip += 1
        lit = token >> 4
        if lit:
            if lit == 15:
                while True:                                 # read_integer (:160-174)
                    if ip >= n:
                        return EXPECTED_ANOTHER_BYTE, out, before
                    x = b[ip]
                    ip += 1
                    lit += x
                    if x != 255:
                        break
            if lit > n - ip:
                return LITERAL_OUT_OF_BOUNDS, out, before   # the FULL length is checked (:346-348)
            m = lit if lit < target - op else target - op
            out += b[ip:ip + m]
            op += m
            ip += lit
            if op == target:
                return OK, out, before
        if ip >= n:
            return OK, out, before                          # :366-368
        if n - ip < 2:
            return EXPECTED_ANOTHER_BYTE, out, before       # :373-375
        off = b[ip] | (b[ip + 1] << 8)
        ip += 2
        if off == 0:
            return OFFSET_ZERO, out, before                 # :168-173
        ml = 4 + (token & 15)
        if ml == 19:
            while True:
                if ip >= n:
                    return EXPECTED_ANOTHER_BYTE, out, before
                x = b[ip]
                ip += 1
                ml += x
                if x != 255:
                    break
        if off > op:
            return OFFSET_OUT_OF_BOUNDS, out, before        # :399-401
        m = ml if ml < target - op else target - op
        start = op - off
        if off >= m:
            out += out[start:start + m]
        else:                                               # byte-serial forward semantics: the period repeats
            out += (bytes(out[start:]) * (m // off + 1))[:m]
        op += m
        if op == target:
            return OK, out, before                          # (no "a match is followed by a token" check here)
        if ip >= n:
            return EXPECTED_ANOTHER_BYTE, out, before       # :439-443
    return OK, out, before


def partial(block, target):
    """(status, bytes): what lz4flex_decompress_batch_partial gives the block at this target -- (0, the first min(size, target) bytes),
    or (the code of the first error the reference meets before `target` bytes exist, b"")"""
    st, out, _ = _run(bytes(block), int(target))
    return (st, bytes(out)) if st == OK else (st, b"")


class Profile:
    """One walk of a block with no target, from which the result at EVERY target follows: status (0 or the block's first error), out (the
    output up to the block's end / up to where the error is raised: P = len(out)), before (the output in front of the sequence the
    error is raised in).  A target t <= P stops the decode before the error is met: at(t) == partial(block, t), which
    tests/test_partial_model.py checks."""

    def __init__(self, block):
        self.empty = len(block) == 0
        self.status, out, self.before = _run(bytes(block), FOREVER)
        self.out = bytes(out)

    def at(self, target):
        if self.empty or (self.status != OK and target > len(self.out)):
            return self.status, b""
        return OK, self.out[:target]


def sequence_starts(block):
    """[(ip, op)] of every sequence of a VALID block: where its token lies and how much output lies in front of it"""
    b, out, ip, op = bytes(block), [], 0, 0
    while ip < len(b):
        out.append((ip, op))
        token = b[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            while b[ip] == 255:
                lit += 255
                ip += 1
            lit += b[ip]
            ip += 1
        ip += lit
        op += lit
        if ip >= len(b):
            break
        ip += 2
        ml = 4 + (token & 15)
        if ml == 19:
            while b[ip] == 255:
                ml += 255
                ip += 1
            ml += b[ip]
            ip += 1
        op += ml
    return out


# ---- blocks written to sit on the paths of the sequence decoder's partial form (lz4_decompress_seq.hip) --------------------------
KEEP, BUDGET, TILE = 1280, 1120, 3840      # the window's history, a chunk's output bytes, a tile's compressed bytes


def _cuts(op0, lit, ml):
    """targets around a sequence that starts at output position op0: inside its literal run, on its last byte, one further, inside its
    match, on its last byte, one further"""
    t = {op0 + 1, op0 + lit // 2, op0 + lit - 1, op0 + lit, op0 + lit + 1, op0 + lit + ml // 2, op0 + lit + ml - 1, op0 + lit + ml,
         op0 + lit + ml + 1}
    return sorted(v for v in t if v > 0)


def writer_cases():
    """[(name, block, plain, targets)]: valid blocks, each with the targets that make one chosen sequence the crossing one (and 0, 1,
    S - 1, S, S + 1 for every block, S its size).  The plain text is the writer's; tests/test_partial_model.py checks it against the
    oracle."""
    from lz4_writer import Writer
    out = []

    def add(name, w, marks, tail=5, cut_after_match=False):
        """marks: (op0, lit, ml) of the sequences to cut around"""
        if cut_after_match:                                  # the block ENDS in a match: valid up to any target <= its size, an error beyond
            c, p = bytes(w.comp), bytes(w.out)
        else:
            c, p = w.end(tail)
        s = len(p)
        t = {0, 1, s - 1, s, s + 1}
        for m in marks:
            t.update(_cuts(*m))
        out.append((name, c, p, sorted(v for v in t if v >= 0)))

    def crossing(w, lit, off, ml, short_behind=3):
        """the sequence, and a few short ones behind it; returns its mark"""
        op0 = len(w.out)
        w.seq(lit, off, ml)
        for _ in range(short_behind):
            w.seq(2, 7, 5)
        return op0, lit, ml

    # ---- the crossing sequence by kind -------------------------------------------------------------------------------------------------
    for lit, ml in ((0, 4), (1, 4), (10, 12), (63, 63), (64, 64)):
        w = Writer(100 + lit)
        w.seq(70, 9, 8)
        add("lane-sized: %d literals, match of %d" % (lit, ml), w, [crossing(w, lit, 66, ml)])
    for lit in (65, 200, 201, 1024, 1025):
        w = Writer(200 + lit)
        w.seq(20, 9, 8)
        add("a literal run of %d" % lit, w, [crossing(w, lit, 11, 9)])
    for off in (1, 2, 3, 15, 16):
        for ml in (5, 40):
            w = Writer(300 + off)
            w.seq(30, 9, 8)
            add("offset %d, match of %d" % (off, ml), w, [crossing(w, 3, off, ml)])
    w = Writer(310)
    w.seq(90, 9, 8)
    add("an offset shorter than the match", w, [crossing(w, 2, 40, 100)])
    for ml in (19, 20, 274):
        w = Writer(320 + ml)
        w.seq(300, 9, 8)
        add("match length %d" % ml, w, [crossing(w, 2, 290, ml)])
    for ml in (16, 17, 64, 65):
        w = Writer(330 + ml)
        w.seq(100, 9, 8)
        for _ in range(500):                                  # 2 500 bytes of output: the block's first bytes have left the window's history
            w.seq(1, 50, 4)
        assert len(w.out) - 100 > KEEP + 200
        add("a far match of %d" % ml, w, [crossing(w, 2, len(w.out) + 2 - 20, ml)])
    # ---- the crossing sequence's place in its chunk --------------------------------------------------------------------------------------
    for k in (0, 1, 62, 63, 64, 65):
        w = Writer(400 + k)
        if k:
            w.seq(40, 9, 8)
            for _ in range(k - 1):
                w.seq(1, 20, 4)
        mark = crossing(w, 30, 10, 20, short_behind=70) if k else crossing(w, 30, 3, 20, short_behind=70)
        add("the crossing sequence is sequence %d" % k, w, [mark])
    for k in (15, 16, 17):                                    # 16 sequences of 70 bytes are the chunk's 1 120: the 17th is cut off by the budget
        w = Writer(420 + k)
        marks = []
        for i in range(24):
            op0 = len(w.out)
            w.seq(2 if i else 66, 70 if i else 66, 68 if i else 4)     # (70 bytes each; the first one puts a source of 68 bytes in front of every match)
            if i == k:
                marks.append((op0, 2, 68))
        add("the byte budget ends at sequence 16, the stop lies in sequence %d" % k, w, marks)
    # ---- tiles and the window ---------------------------------------------------------------------------------------------------------------
    w = Writer(430)
    w.seq(40, 9, 8)
    while len(w.comp) < TILE + 300:
        w.seq(1, 20, 4)
    add("a stop in the second tile", w, [crossing(w, 12, 30, 25)])
    w = Writer(431)
    w.seq(40, 9, 8)
    while len(w.comp) < TILE - 14:
        w.seq(1, 20, 4)
    assert TILE - 16 <= len(w.comp) < TILE
    add("a stop in the last 16 bytes of a tile", w, [crossing(w, 12, 30, 25)])
    w = Writer(432)
    w.seq(40, 9, 8)
    while len(w.out) < 3584 + 200:
        w.seq(1, 20, 4)
    assert len(w.comp) < TILE
    add("a stop behind a window slide", w, [crossing(w, 12, 30, 25)])
    # ---- a match that ends the block: valid at every target up to its end ("no token behind it"), ExpectedAnotherByte beyond ---------------
    for lit, off, ml in ((3, 9, 6), (0, 2, 30), (70, 50, 300)):
        w = Writer(440 + ml)
        w.seq(60, 9, 8).seq(2, 7, 5)
        op0 = len(w.out)
        w.seq(lit, off, ml)
        add("the block ends in a match of %d" % ml, w, [(op0, lit, ml)], cut_after_match=True)
    return out


def corrupted_cases():
    """[(name, block, targets)]: one damaged place per block -- an offset of 0, an offset one past the output, the input cut inside a
    match length run, the input cut inside a literal run -- in front of the stop, in the crossing sequences, right behind them (same
    tile) and a tile later.  Every place holds two sequences of 6 literals and a match of 30 (one length byte): A with offset 9 (one
    byte makes it 0), B with an offset that reaches the output's first byte (one more is one too many).  The targets put the stop into
    the literals and into the match of the second place's A and B."""
    from lz4_writer import Writer
    w = Writer(500)
    w.seq(20, 9, 8)
    place = {}

    def victims(name):
        a = len(w.comp)
        w.seq(6, 9, 30)
        b, op = len(w.comp), len(w.out)
        assert (op + 6) & 0xFF != 0xFF
        w.seq(6, op + 6, 30)
        place[name] = (a, b, op - 36)
        w.seq(2, 7, 5)

    victims("in front of the stop")
    victims("the crossing sequence")
    victims("right behind the stop")
    while len(w.comp) < place["right behind the stop"][0] + TILE + 100:
        w.seq(1, 20, 4)
    victims("a tile later")
    comp = w.end(5)[0]
    cop = place["the crossing sequence"][2]                   # where its A starts in the output; its B starts 36 bytes further
    targets = [0, 1] + [cop + d for d in (3, 6, 17, 36, 39, 42, 53, 72, 73)] + [len(w.out), len(w.out) + 9]
    out = []
    for name, (a, b, _) in place.items():
        zero, past = bytearray(comp), bytearray(comp)
        assert zero[a + 7] == 9 and zero[a + 8] == 0          # token, 6 literals, then the offset
        zero[a + 7] = 0
        past[b + 7] += 1
        out.append(("offset 0, " + name, bytes(zero), targets))
        out.append(("an offset one past the output, " + name, bytes(past), targets))
        out.append(("the input cut inside a match length run, " + name, comp[:a + 9], targets))
        out.append(("the input cut inside a literal run, " + name, comp[:a + 4], targets))
    return out
