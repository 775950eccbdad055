"""Damaged and truncated frames for tests/test_gpu_frame_damage.py, made from the oracle alone (nothing of the library is imported).

The content is four 64 KiB-mode blocks: JSON (compressed), random bytes (stored), text (compressed) and a short tail that repeats the
end of the text block (in a Linked frame it refers back into its predecessor).  Four blocks are the fewest at which the reference's
Linked decoder has wrapped its ring of 2 * 65 536 + 65 536 bytes (src/frame/decompress.rs:145-156,202-211): the last block is decoded
against an external dictionary, into a sink that ends where that dictionary starts.

Eight base frames (block mode x block checksums x content checksum and size), written by the oracle's FrameEncoder.  cases(key) gives
a base frame's cases as (name, bytes, out_cap, k): k is the first block whose BlockInfo word, payload or checksum holds the first
damaged or missing byte, 0 for damage in the header and `blocks` for damage at or behind the EndMark.  A name starts with its
family: flip, cut, header, info, block, around, sink.  tests/test_frame_damage_cases.py holds the census of what the oracle says about
them."""
import functools
import struct

import numpy as np

import frame_index_cases as FC
import oracle_api as O

BLOCK = 65536
TAIL = 20000
CONTENT_LEN = 3 * BLOCK + TAIL
SLACK = 70000
STORED = 0x80000000
LEGACY_MAGIC = 0x184C2102
FAMILIES = ("flip", "cut", "header", "info", "block", "around", "sink")

# (key, block_mode, block_checksums, content checksum and content size)
BASES = [("%s-%s-%s" % ("lnk" if mode else "ind", "bsum" if bc else "nosum", "csum+size" if cc else "bare"), mode, bc, cc)
         for mode in (0, 1) for bc in (False, True) for cc in (False, True)]
KEYS = [b[0] for b in BASES]


@functools.lru_cache(maxsize=None)
def content():
    json = O.fixture_plain("compression_66k_JSON")[:BLOCK]
    rnd = np.random.default_rng(3).integers(0, 256, BLOCK, dtype=np.uint8).tobytes()
    text = O.fixture_plain("compression_65k")
    text = (text + text)[:BLOCK]                          # (the fixture is 64 723 bytes: its start again fills the block)
    assert len(json) == len(text) == BLOCK
    out = json + rnd + text + text[-TAIL:]
    assert len(out) == CONTENT_LEN
    return out


class Base:
    """a base frame and where its parts lie: header_len, info_off[k] (BlockInfo words), payload[k] = (offset, length), sum_off[k]
    (block checksums, [] without), end_off (EndMark), csum_off (content checksum or None), content_off[0 .. blocks]"""

    def __init__(self, key, mode, block_checksums, sized):
        self.key, self.mode, self.block_checksums, self.sized = key, mode, block_checksums, sized
        kw = dict(block_size=4, block_mode=mode, block_checksums=block_checksums, content_checksum=sized)
        if sized:
            kw["content_size"] = CONTENT_LEN
        rc, f = O.frame_compress(content(), **kw)
        assert rc == 0
        self.frame = f
        self.header_len = 7 + (8 if sized else 0)
        self.info_off, self.payload, self.sum_off, self.words = [], [], [], []
        p = self.header_len
        while True:
            (w,) = struct.unpack_from("<I", f, p)
            if w == 0:
                break
            n = w & ~STORED
            self.info_off.append(p); self.words.append(w); self.payload.append((p + 4, n))
            p += 4 + n
            if block_checksums:
                self.sum_off.append(p); p += 4
        self.end_off = p
        self.csum_off = p + 4 if sized else None
        assert len(f) == p + 4 + (4 if sized else 0)
        self.blocks = len(self.info_off)
        self.content_off = [min(k * BLOCK, CONTENT_LEN) for k in range(self.blocks)] + [CONTENT_LEN]
        assert self.blocks == 4 and [bool(w & STORED) for w in self.words] == [False, True, False, False]

    def block_of(self, off):
        """the k of a damaged or missing byte at frame offset `off`"""
        if off < self.header_len:
            return 0
        if off >= self.end_off:
            return self.blocks
        return max(k for k in range(self.blocks) if self.info_off[k] <= off)


@functools.lru_cache(maxsize=None)
def base(key):
    return Base(*BASES[KEYS.index(key)])


def repair(header):
    """the header with its HC byte recomputed, so that the check behind the checksum is reached"""
    h = bytearray(header)
    h[-1] = (O.xxh32(bytes(h[4:-1])) >> 8) & 0xFF
    return bytes(h)


def _flips(b):
    f = b.frame
    spans = [(0, b.header_len)]
    spans += [(o, 4) for o in b.info_off] + [(o, 4) for o in b.sum_off] + [(b.end_off, 4)]
    if b.csum_off is not None:
        spans.append((b.csum_off, 4))
    at = {}
    for lo, n in sorted(spans):
        for o in range(lo, lo + n):
            at.setdefault(o, []).extend((0x01, 0x80))
    for po, n in b.payload:
        for o in list(range(po, po + min(24, n))) + list(range(po + max(n - 8, 0), po + n)):
            if 0x5A not in at.setdefault(o, []):
                at[o].append(0x5A)
    for o in range(0, len(f), 509):
        if 0x5A not in at.setdefault(o, []):
            at[o].append(0x5A)
    for o in sorted(at):
        for x in at[o]:
            g = bytearray(f); g[o] ^= x
            yield "flip %d^%02x" % (o, x), bytes(g), b.block_of(o)


def _cuts(b):
    f = b.frame
    n = len(f)
    ls = set(range(0, b.header_len + 7))
    for m in b.info_off + [b.end_off]:
        ls.update((m - 1, m, m + 1, m + 3, m + 4, m + 5))
    ls.update(range(n - 10, n))
    ls.update(range(0, n, 1013))
    for length in sorted(v for v in ls if 0 <= v < n):
        yield "cut %d" % length, f[:length], b.block_of(length)


def _headers(b):
    f = b.frame
    h, rest = f[:b.header_len], f[b.header_len:]
    out = []
    for bit in range(8):
        g = bytearray(h); g[4] ^= 1 << bit
        if bit == 0:                                         # a dictionary id appears: its four bytes with it
            g[-1:-1] = b"\0\0\0\0"
        if bit == 3:                                         # the content size goes or appears: its eight bytes with it
            g[6:-1] = b"" if b.sized else struct.pack("<Q", CONTENT_LEN)
        out.append(("header flg bit %d" % bit, repair(g) + rest))
        g = bytearray(h); g[5] ^= 1 << bit
        out.append(("header bd bit %d" % bit, repair(g) + rest))
    for bs in range(8):
        g = bytearray(h); g[5] = (g[5] & 0x8F) | (bs << 4)
        out.append(("header block size %d" % bs, repair(g) + rest))
    for v in (0, 2, 3):
        g = bytearray(h); g[4] = (g[4] & 0x3F) | (v << 6)
        out.append(("header version %d" % v, repair(g) + rest))
    g = bytearray(h); g[4] |= 0x01
    out.append(("header dictionary id", repair(bytes(g[:-1]) + b"\x11\x22\x33\x44" + bytes(g[-1:])) + rest))
    if b.sized:
        for d in (-1, 1):
            g = bytearray(h); struct.pack_into("<Q", g, 6, CONTENT_LEN + d)
            out.append(("header content size %+d" % d, repair(g) + rest))
    for name, data in out:
        yield name, data, 0


def _infos(b):
    f = b.frame
    for k in range(b.blocks):
        w = b.words[k]
        n = w & ~STORED
        for tag, v in (("-1", (w & STORED) | (n - 1)), ("+1", (w & STORED) | (n + 1)), ("65537", (w & STORED) | 65537),
                       ("7fffffff", 0x7FFFFFFF), ("0", 0), ("80000000", STORED)):
            g = bytearray(f); struct.pack_into("<I", g, b.info_off[k], v)
            yield "info %d = %s" % (k, tag), bytes(g), k


@functools.lru_cache(maxsize=None)
def too_big_block():
    """a valid block that decodes to block size + 1 bytes, and a short one: a literal and one long match"""
    blk = O.compress(bytes(BLOCK + 1))
    assert len(blk) < 280
    return blk


def _replaced(b):
    f = b.frame
    new = (("65537 bytes", too_big_block(), 0), ("0 bytes", b"\x00", 0), ("offset zero", FC.offset_zero_block(), 0),
           ("stored 0 bytes", b"", STORED))
    for k in (1, 3):
        lo = b.info_off[k]
        hi = b.payload[k][0] + b.payload[k][1] + (4 if b.block_checksums else 0)
        for tag, pay, stored in new:
            blk = struct.pack("<I", len(pay) | stored) + pay + (struct.pack("<I", O.xxh32(pay)) if b.block_checksums else b"")
            yield "block %d -> %s" % (k, tag), f[:lo] + blk + f[hi:], k


def _around(b):
    f = b.frame
    for magic in (0x184D2A50, 0x184D2A5F):
        yield "around skippable %08x" % magic, struct.pack("<II", magic, 5) + b"12345" + f, 0
    rc, second = O.frame_compress(b"a second frame", block_size=4)
    assert rc == 0
    yield "around second frame", f + second, b.blocks
    yield "around garbage behind", f + b"\xde\xad\xbe\xef\x01\x02\x03\x04", b.blocks
    yield "around legacy magic", struct.pack("<I", LEGACY_MAGIC) + f[b.header_len:], 0
    yield "around empty", b"", 0
    yield "around magic alone", f[:4], 0


def _sinks(b):
    for cap in (0, b.content_off[2], b.content_off[2] + 1, CONTENT_LEN - 1, CONTENT_LEN):
        yield "sink %d" % cap, b.frame, cap, b.blocks


def cases(key):
    """[(name, bytes, out_cap, k)] of a base frame; the same list on every call"""
    b = base(key)
    out = []
    for gen in (_flips, _cuts, _headers, _infos, _replaced, _around):
        out += [(name, data, CONTENT_LEN + SLACK, k) for name, data, k in gen(b)]
    out += list(_sinks(b))
    return out


def family(name):
    return name.split(" ", 1)[0]


# ---- what the oracle says: computed once per base frame by the tests that need it, and left alone
class Verdict:
    """the oracle's frame_decompress of a case: code (0 or the error's number), detail (expected, actual, inner), consumed, and on
    success out_len and the bytes (`prefix`: they are content()[:out_len], kept as that to spare memory; else `data` holds them)"""
    __slots__ = ("code", "detail", "consumed", "out_len", "prefix", "data")

    def output(self):
        return content()[:self.out_len] if self.prefix else self.data


def verdict(data, out_cap):
    v = Verdict()
    rc, res, v.consumed = O.frame_decompress(data, out_cap)
    v.code, v.detail, v.out_len, v.prefix, v.data = rc, (0, 0, 0), 0, True, None
    if rc:
        v.detail = res
    else:
        v.out_len = len(res)
        v.prefix = res == content()[:len(res)]
        v.data = None if v.prefix else res
    return v


# ---- where lz4flex_frame_index_create answers otherwise than the oracle, as include/lz4flex_amd.h states in words: rules over case
# families, counted by tests/test_frame_damage_cases.py.  (The decoders have none.)
HEADER_CODES = (18, 19, 20, 21, 22, 25, 28, 29)
def reader_waits(name, v):
    """include/lz4flex_amd.h, lz4flex_frame_index_create: "a truncated frame (-LZ4FLEX_FE_IO; also one that ends where its EndMark should
    be, which a streaming reader takes for "no more bytes yet", src/frame/decompress.rs:231-238)".  The cuts the oracle answers 0 for
    although bytes are missing -- the frame ends at or inside a BlockInfo or EndMark word, or with its magic number (v: the cut's
    verdict) -- have no index: -LZ4FLEX_FE_IO."""
    return family(name) == "cut" and v.code == 0


def reads_as_linked(name, data, v):
    """include/lz4flex_amd.h, lz4flex_frame_index_create: "-LZ4FLEX_E_UNSUPPORTED: BlockMode::Linked frames (a block needs the 64 KiB in
    front of it, transitively: there is nothing to seek in)".  A repaired header whose FLG byte says Linked and that parses (v: its
    verdict is no header error) has no index: -LZ4FLEX_E_UNSUPPORTED."""
    return family(name) == "header" and not data[4] & 0x20 and not (v.code in HEADER_CODES and v.consumed == 0)


def delivered(data, out_cap):
    """the bytes the oracle's reader had handed out when it stopped, error or not: what two runs over differently filled buffers both wrote"""
    import ctypes as C
    runs = []
    for fill in (0x11, 0xEE):
        out = C.create_string_buffer(max(out_cap, 1))
        C.memset(out, fill, max(out_cap, 1))
        used, d = C.c_size_t(0), O.ErrDetail()
        O.lib().lz4o_frame_decompress(bytes(data), len(data), out, out_cap, C.byref(used), C.byref(d))
        runs.append(out.raw[:out_cap])
    a, b = np.frombuffer(runs[0], np.uint8), np.frombuffer(runs[1], np.uint8)
    diff = np.flatnonzero(a != b)
    return runs[0][:int(diff[0]) if len(diff) else out_cap]


def checksum_twin(data):
    """the same frame with no checksum wrong: every block checksum rewritten to fit its payload as far as the BlockInfo words lead, the
    content-checksum flag cleared (the bytes behind the EndMark are then not read) and the header's HC byte recomputed.  For what
    lz4flex_frame_index_create promises, "as lz4flex_frame_decompress does for the same bytes when no checksum is wrong": the oracle's
    verdict on the twin is what "a content that differs but is structurally sound succeeds" asks of create, as an exact value."""
    g = bytearray(data)
    flg = g[4]
    hl = 7 + (8 if flg & 0x08 else 0)
    if flg & 0x10:
        p = hl
        while p + 4 <= len(g):
            (w,) = struct.unpack_from("<I", g, p)
            n = w & ~STORED
            if w == 0 or p + 4 + n + 4 > len(g):
                break
            struct.pack_into("<I", g, p + 4 + n, O.xxh32(bytes(g[p + 4:p + 4 + n])))
            p += 8 + n
    g[4] = flg & ~0x04 & 0xFF
    g[:hl] = repair(g[:hl])
    return bytes(g)
