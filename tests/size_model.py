"""A pure-Python model of lz4flex_decompressed_size_batch (lz4_size_scan.hip): src/block/decompress.rs:201-449 with an unbounded sink,
lengths only.  tests/test_size_scan_model.py pins it to the oracle; the GPU tests (tests/test_gpu_size_scan.py) check the kernels
against it."""

OK, LITERAL_OUT_OF_BOUNDS, EXPECTED_ANOTHER_BYTE, OFFSET_ZERO, OFFSET_OUT_OF_BOUNDS = 0, 2, 3, 4, 5
NAMES = {LITERAL_OUT_OF_BOUNDS: "LiteralOutOfBounds", EXPECTED_ANOTHER_BYTE: "ExpectedAnotherByte", OFFSET_ZERO: "OffsetZero",
         OFFSET_OUT_OF_BOUNDS: "OffsetOutOfBounds"}


class _Err(Exception):
    def __init__(self, code):
        self.code = code


def _read_integer(b, ip):
    """read_integer (:160-174): (value, ip behind it)"""
    v = 0
    while True:
        if ip >= len(b):
            raise _Err(EXPECTED_ANOTHER_BYTE)
        x = b[ip]
        ip += 1
        v += x
        if x != 255:
            return v, ip


def size(block, history=0):
    """(status, new bytes): what decompress_into would return with `history` bytes in front of the block's output and no capacity
    limit; (code, 0) for an error"""
    b = bytes(block)
    n = len(b)
    if n == 0:
        return EXPECTED_ANOTHER_BYTE, 0                     # :207-209
    ip = op = 0
    try:
        while True:
            token = b[ip]
            ip += 1
            lit = token >> 4
            if lit:
                if lit == 15:
                    v, ip = _read_integer(b, ip)
                    lit += v
                if lit > n - ip:
                    return LITERAL_OUT_OF_BOUNDS, 0         # :346-348
                op += lit
                ip += lit
            if ip >= n:
                return OK, op                               # :366-368
            if n - ip < 2:
                return EXPECTED_ANOTHER_BYTE, 0             # :373-375
            off = b[ip] | (b[ip + 1] << 8)
            ip += 2
            if off == 0:
                return OFFSET_ZERO, 0                       # :168-173
            ml = 4 + (token & 15)
            if ml == 19:
                v, ip = _read_integer(b, ip)
                ml += v
            if off > op + history:
                return OFFSET_OUT_OF_BOUNDS, 0              # :399-401
            op += ml
            if ip >= n:
                return EXPECTED_ANOTHER_BYTE, 0             # :439-443
    except _Err as e:
        return e.code, 0


def writer_cases():
    """[(name, block, history)] written with lz4_writer.Writer to sit on the size scan's boundaries: runs of 255 length bytes, literal
    runs around the lane / walk limits (192 / 200 bytes), blocks that end in a match, offsets exactly as far back as the output reaches
    and one byte further"""
    from lz4_writer import Writer
    out = []
    w = Writer(1)
    w.seq(1, 1, 1 << 20)
    out.append(("4 KiB of 255 length bytes, 1 MiB of output", w.end(5)[0], 0))
    w = Writer(2)
    w.seq(70000, 1, 100).seq(3, 50, 300000)
    out.append(("a 70 000-byte literal run and a 300 000-byte match", w.end(1000)[0], 0))
    for lit in (191, 192, 193, 199, 200, 201, 254, 269, 270, 271, 525):
        w = Writer(3 + lit)
        for k in range(40):
            w.seq(lit if k % 3 == 0 else 5, 1 + (k % 7), 4 + k)
        out.append(("literal runs of %d bytes" % lit, w.end(lit)[0], 0))
    for ml in (18, 19, 20, 273, 274, 275, 529):
        w = Writer(30 + ml)
        for k in range(70):
            w.seq(k % 4 + 3, 1 + k % 3, ml if k % 2 else 4)
        c = w.end(7)[0]
        out.append(("match lengths of %d" % ml, c, 0))
        out.append(("match lengths of %d, ending in a match" % ml, c[:-8], 0))
    for k in (1, 3, 40):
        w = Writer(50 + k)
        for _ in range(k):
            w.seq(3, 2, 6)
        out.append(("%d sequences, no last literals" % k, bytes(w.comp), 0))
    for hist in (0, 1, 16, 1000, 65000):
        for lit in (0, 5, 300):
            if hist + lit < 1 or hist + lit + 1 > 65535:
                continue
            prefix = bytes(hist)
            w = Writer(60 + lit, prefix)
            w.seq(lit, hist + lit, 4)
            out.append(("offset = history %d + position %d" % (hist, lit), w.end(5)[0], hist))
            w = Writer(60 + lit, prefix)
            w.bad_seq(lit, hist + lit + 1, 4)
            out.append(("offset = history %d + position %d + 1" % (hist, lit), w.end(5)[0], hist))
    # far into a block: many chunks of sequences, then an offset one byte past everything (the check in the 64-lane chunks)
    w = Writer(77)
    for k in range(3000):
        w.seq(k % 9 + 1, 1 + (k * 7) % min(50, len(w.out) + 1), 4 + k % 20)
    pos = len(w.out)
    w.bad_seq(2, pos + 3, 4)
    out.append(("offset one byte past the output, after 3 000 sequences", w.end(5)[0], 0))
    out.append(("... the same with one byte of history", out[-1][1], 1))
    return out
