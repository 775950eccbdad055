"""A pure-Python model of lz4flex_decompress_batch_partial_shared_dict / _dict_set (include/lz4flex_amd.h, "PARTIAL DECODE AGAINST A
DICTIONARY"): the walk of tests/partial_model.py with two changes -- the output starts as the dictionary's last min(len, 65 536) bytes
(copy_from_dict, src/block/decompress.rs:85-109 / :410-426, reads nothing older: an offset is at most 65 535), and the offset check is
offset > op + len(dictionary), the UNTRUNCATED length (:399-401).  tests/test_partial_dict_model.py pins it to the oracle; the GPU tests
(tests/test_gpu_partial_dict.py) check the kernels against it.  The case generators below write blocks whose offsets reach into the
dictionary, on the paths of the sequence decoder's form with a dictionary and a target (lz4_decompress_seq.hip Dec<G, true, true>)."""
from partial_model import FOREVER, KEEP, TILE, _cuts
from size_model import EXPECTED_ANOTHER_BYTE, LITERAL_OUT_OF_BOUNDS, OFFSET_OUT_OF_BOUNDS, OFFSET_ZERO, OK

WINDOW = 65536        # what a decoder reads of a dictionary: its last 64 KiB
DICT_LENGTHS = (1, 15, 16, 17, 1279, 1280, 1281, 4096, 65535, 65536, 70001)     # either side of: PV's rounding to 16, the KEEP window
#                   reload, the 64 KiB truncation, "the untruncated length is the one in the offset check"


def dictionary(length, seed=7):
    """`length` bytes that repeat nowhere within a match's reach: a wrong source position gives wrong bytes"""
    import random
    return random.Random(seed * 1000003 + length).randbytes(length)


def _run(b, target, dic):
    """partial_model._run with the dictionary: (status, the block's output so far, its bytes in front of the sequence the walk ended in)"""
    n, dl = len(b), len(dic)
    if n == 0:
        return EXPECTED_ANOTHER_BYTE, bytearray(), 0        # :207-209, before anything else
    out = bytearray(dic[-WINDOW:]) if dl else bytearray()
    base = len(out)
    ip = op = before = 0                                    # (op == len(out) - base)
    while op < target:
        before = op
        token = b[ip]
        ip += 1
        lit = token >> 4
        if lit:
            if lit == 15:
                while True:
                    if ip >= n:
                        return EXPECTED_ANOTHER_BYTE, out[base:], before
                    x = b[ip]
                    ip += 1
                    lit += x
                    if x != 255:
                        break
            if lit > n - ip:
                return LITERAL_OUT_OF_BOUNDS, out[base:], before
            m = lit if lit < target - op else target - op
            out += b[ip:ip + m]
            op += m
            ip += lit
            if op == target:
                return OK, out[base:], before
        if ip >= n:
            return OK, out[base:], before
        if n - ip < 2:
            return EXPECTED_ANOTHER_BYTE, out[base:], before
        off = b[ip] | (b[ip + 1] << 8)
        ip += 2
        if off == 0:
            return OFFSET_ZERO, out[base:], before
        ml = 4 + (token & 15)
        if ml == 19:
            while True:
                if ip >= n:
                    return EXPECTED_ANOTHER_BYTE, out[base:], before
                x = b[ip]
                ip += 1
                ml += x
                if x != 255:
                    break
        if off > op + dl:
            return OFFSET_OUT_OF_BOUNDS, out[base:], before     # :399-401: the dictionary's whole length counts
        m = ml if ml < target - op else target - op
        start = len(out) - off                              # (>= 0: off <= 65 535, and off <= op + dl)
        if off >= m:
            out += out[start:start + m]
        else:                                               # byte-serial forward semantics: the period repeats
            out += (bytes(out[start:]) * (m // off + 1))[:m]
        op += m
        if op == target:
            return OK, out[base:], before                   # (no "a match is followed by a token" check here)
        if ip >= n:
            return EXPECTED_ANOTHER_BYTE, out[base:], before
    return OK, out[base:], before


def partial_with_dict(block, target, dictionary):
    """(status, bytes): what the entries give the block at this target against this dictionary -- (0, the first min(size, target)
    bytes), or (the code of the first error the reference meets before `target` bytes exist, b"")"""
    st, out, _ = _run(bytes(block), int(target), bytes(dictionary))
    return (st, bytes(out)) if st == OK else (st, b"")


class Profile:
    """partial_model.Profile with a dictionary: one walk with no target, from which the result at every target follows"""

    def __init__(self, block, dictionary):
        self.empty = len(block) == 0
        self.status, out, self.before = _run(bytes(block), FOREVER, bytes(dictionary))
        self.out = bytes(out)

    def at(self, target):
        if self.empty or (self.status != OK and target > len(self.out)):
            return self.status, b""
        return OK, self.out[:target]


# ---- blocks whose matches reach into the dictionary -------------------------------------------------------------------------------
def _writer(seed, dic):
    from lz4_writer import Writer
    return Writer(seed, prefix=dic[-WINDOW:])


def dict_cases(dic):
    """[(name, block, plain, targets)] against the dictionary `dic` (at least one byte): valid blocks (those named "the block ends in
    ..." are valid up to their size and ExpectedAnotherByte beyond), each with 0, 1, S - 1, S, S + 1 and the targets around its marked
    sequences.  The plain text is the writer's; tests/test_partial_dict_model.py checks it against the oracle."""
    win = min(len(dic), WINDOW)
    reach = min(win, 65535)                                   # the oldest byte an offset reaches from op = 0
    out = []

    def add(name, w, marks, extra=(), cut_after_match=False):
        if cut_after_match:                                  # the block ENDS in a match: valid at EVERY target up to its size, an error beyond
            c, p = bytes(w.comp), bytes(w.out[w.base:])
            extra = set(extra) | set(range(len(p) + 2))
        else:
            c, p = w.end(5)
        s = len(p)
        t = {0, 1, s - 1, s, s + 1} | set(extra)
        for m in marks:
            t.update(_cuts(*m))
        out.append((name, c, p, sorted(v for v in t if v >= 0)))

    def behind(w):
        for _ in range(3):
            w.seq(2, 7, 5)

    # ---- the first sequence, no literals, the match's source starts in the dictionary --------------------------------------------
    for ml in (4, 16, 17, 64, 65, 300, 1023, 1024, 1025, 2000):
        for off in sorted({1, max(reach // 2, 1), reach}):
            w = _writer(1000 + ml + off, dic)
            w.seq(0, off, ml)
            behind(w)
            add("first sequence: offset %d of %d, match of %d" % (off, reach, ml), w, [(0, 0, ml)])
    # ---- straddling matches: the source starts k bytes in front of the dictionary's end ---------------------------------------------
    for k in (1, 3, 15, 16, 17, 63, 64):
        if k > reach:
            continue
        for ml in (k + 1, k + 20, 2 * k + 5):
            for lit in (0, 24):                               # (0: everything behind the dictionary part is the match's own output)
                if ml < 4:
                    continue
                w = _writer(1100 + 7 * k + ml + lit, dic)
                w.seq(lit, lit + k, ml)
                behind(w)
                m0 = lit
                extra = {m0 + max(k // 2, 1), m0 + k - 1, m0 + k, m0 + k + 1, m0 + k + (ml - k + 1) // 2, m0 + ml, m0 + ml + 1}
                add("straddling: %d literals, %d bytes of dictionary, match of %d" % (lit, k, ml), w, [(0, lit, ml)], extra)
    # ---- far matches: the source has left the window's history and lies in the dictionary ---------------------------------------------
    for j in (10, 40, 64, 200):                               # [src, src + 64) crosses the dictionary's end (j < 64) or does not
        if j > reach:
            continue
        for ml in (16, 17, 64, 65):
            w = _writer(1200 + j + ml, dic)
            w.seq(100, 9, 8)
            for _ in range(500):
                w.seq(1, 50, 4)
            op0 = len(w.out) - w.base
            assert op0 > KEEP + 200 and op0 + 2 + j <= 65535
            w.seq(2, op0 + 2 + j, ml)
            behind(w)
            add("far: the source starts %d bytes in front of the dictionary's end, match of %d" % (j, ml), w, [(op0, 2, ml)])
    # ---- long runs clipped by the target: 1 023, 1 024, 1 025 and 1 500 bytes of them -------------------------------------------------
    for off in sorted({min(3, reach), min(100, reach)} | {o for o in (1024, 3000) if o <= reach}):     # (from 1 024 on: memory to memory)
        for lit in (0, 5):
            w = _writer(1300 + off + lit, dic)
            w.seq(lit, lit + off, 2000)
            behind(w)
            add("a long run: %d literals, offset %d into the dictionary" % (lit, off), w, [(0, lit, 2000)],
                {lit + c for c in (1023, 1024, 1025, 1500)})
    # ---- blocks that end in a match -------------------------------------------------------------------------------------------------------
    if reach >= 6:
        w = _writer(1400, dic)
        w.seq(4, 4 + min(reach, 40), 6)
        add("the block ends in a match from the dictionary", w, [(0, 4, 6)], cut_after_match=True)
    w = _writer(1401, dic)
    k = min(reach, 5)
    w.seq(4, 4 + k, k + 9)
    add("the block ends in a straddling match", w, [(0, 4, k + 9)], {4 + k - 1, 4 + k, 4 + k + 1}, cut_after_match=True)
    return out


def damaged_cases(dic):
    """[(name, block, targets)]: partial_model.corrupted_cases' layout against `dic` -- four places of two sequences (6 literals and a
    match of 30 each): A with offset 9 (one byte makes it 0), B with an offset that reaches the dictionary's OLDEST byte the untruncated
    length allows (one more is one too many).  Dictionaries of 65 535 bytes and more: every offset there is lies inside, B takes the
    largest one, and there is no "one past" damage."""
    dl = len(dic)
    w = _writer(1500, dic)
    w.seq(20, 9, 8)
    place = {}
    can_pass = dl < 65535

    def victims(name):
        a, opa = len(w.comp), len(w.out) - w.base
        w.seq(6, 9, 30)
        while can_pass and (len(w.out) - w.base + 6 + dl) & 0xFF == 0xFF:     # (the damage adds one to the offset's low byte)
            w.seq(1, 7, 4)
        b, op = len(w.comp), len(w.out) - w.base
        w.seq(6, min(op + 6 + dl, 65535), 30)
        place[name] = (a, b, opa)
        w.seq(2, 7, 5)

    victims("in front of the stop")
    victims("the crossing sequence")
    victims("right behind the stop")
    while len(w.comp) < place["right behind the stop"][0] + TILE + 100:
        w.seq(1, 20, 4)
    victims("a tile later")
    comp, plain = w.end(5)
    cop = place["the crossing sequence"][2]                   # where its A starts in the output; its B starts 36 bytes further (or 41)
    targets = [0, 1] + [cop + d for d in (3, 6, 17, 36, 39, 42, 44, 47, 53, 58, 72, 73, 78)] + [len(plain), len(plain) + 9]
    out = []
    for name, (a, b, _) in place.items():
        zero = bytearray(comp)
        assert zero[a + 7] == 9 and zero[a + 8] == 0
        zero[a + 7] = 0
        out.append(("offset 0, " + name, bytes(zero), targets))
        if can_pass:
            past = bytearray(comp)
            past[b + 7] += 1
            out.append(("an offset one past the dictionary, " + name, bytes(past), targets))
    return out
