"""Frames for the frame-index tests, written block by block in plain Python: the header is the oracle encoder's, each block is a
BlockInfo word + payload (+ XXH32 of the payload), then the EndMark (+ XXH32 of the content).  A payload is the oracle's
compress(piece), or the piece itself when that did not shrink (the reference's store-raw rule, src/frame/compress.rs:301-306).
Unlike the oracle's own encoder -- whose `chunks` are write sizes, not flushes -- this writes short blocks in the middle of a frame.
tests/test_frame_index_cases.py holds every frame made here against the oracle's FrameDecoder."""
import struct

import corpus
import oracle_api as O

STORED = 0x80000000
BLOCK = 65536


class Written:
    """frame: the bytes; pieces: the content, block by block; content_off / payload_off / len_word: what an index of it holds"""

    def __init__(self, frame, pieces, content_off, payload_off, len_word, block_checksums):
        self.frame, self.pieces, self.content_off, self.payload_off, self.len_word = frame, pieces, content_off, payload_off, len_word
        self.block_checksums = block_checksums
        self.content = b"".join(pieces)

    @property
    def stored(self):
        return [bool(w & STORED) for w in self.len_word]


def header(content, **kw):
    """the oracle encoder's header for a frame of this content"""
    rc, f = O.frame_compress(content, **kw)
    assert rc == 0
    return f[:7 + (8 if kw.get("content_size") is not None else 0)]


def write_frame(pieces, block_checksums=False, content_checksum=False, with_content_size=False, block_size=4, payloads=None):
    """payloads: {block index: (payload bytes, stored)} replaces what the rule above gives that block"""
    content = b"".join(pieces)
    kw = dict(block_size=block_size, block_checksums=block_checksums, content_checksum=content_checksum)
    if with_content_size:
        kw["content_size"] = len(content)
    out = bytearray(header(content, **kw))
    content_off, payload_off, len_word, at = [0], [], [], 0
    for i, piece in enumerate(pieces):
        comp = O.compress(piece)
        pay, stored = (comp, False) if len(comp) < len(piece) else (piece, True)
        if payloads and i in payloads:
            pay, stored = payloads[i]
        word = len(pay) | (STORED if stored else 0)
        out += struct.pack("<I", word)
        payload_off.append(len(out)); len_word.append(word)
        out += pay
        if block_checksums:
            out += struct.pack("<I", O.xxh32(pay))
        at += len(piece); content_off.append(at)
    out += struct.pack("<I", 0)
    if content_checksum:
        out += struct.pack("<I", O.xxh32(content))
    return Written(bytes(out), list(pieces), content_off, payload_off, len_word, block_checksums)


def text():
    t = O.fixture_plain("compression_66k_JSON")
    while len(t) < 6 * BLOCK:
        t += t
    return t


def rand():
    return corpus.lcg_bytes(BLOCK, 4711)


def seven_pieces():
    t, r = text(), rand()
    return [t[:100], t[:65536], t[:1], r[:65536], r[:7], t[5:65536], t[:40000]]


SEVEN_STORED = [False, False, True, True, True, False, False]


def seven(block_checksums=False):
    """7 blocks: compressed, compressed-full, stored 1 byte, stored full, stored 7 bytes, compressed, a compressed last block"""
    w = write_frame(seven_pieces(), block_checksums=block_checksums)
    assert w.stored == SEVEN_STORED
    return w


def walk(frame, block_checksums, header_len):
    """(payload_off, len_word, offset behind the EndMark) of a well-formed frame"""
    po, lw, p = [], [], header_len
    while True:
        (w,) = struct.unpack_from("<I", frame, p)
        p += 4
        if w == 0:
            return po, lw, p
        po.append(p); lw.append(w)
        p += (w & ~STORED) + (4 if block_checksums else 0)


def oracle_frame(content, **kw):
    """a frame of the oracle's encoder as a Written (its blocks are full but the last)"""
    rc, f = O.frame_compress(content, **kw)
    assert rc == 0
    bs = {4: 65536, 5: 262144, 6: 1 << 20, 7: 4 << 20}[kw.get("block_size", 4)]
    pieces = [content[i:i + bs] for i in range(0, len(content), bs)]
    hl = 7 + (8 if kw.get("content_size") is not None else 0)
    po, lw, _ = walk(f, kw.get("block_checksums", False), hl)
    co = [0]
    for p in pieces:
        co.append(co[-1] + len(p))
    assert len(po) == len(pieces)
    return Written(f, pieces, co, po, lw, kw.get("block_checksums", False))


def plain_oracle():
    """about 5 full blocks and a remainder"""
    return oracle_frame(text()[:5 * BLOCK + 12345], block_size=4)


def sized_oracle():
    """content size and content checksum in the frame"""
    c = text()[1000:1000 + 150000]
    return oracle_frame(c, block_size=4, content_size=len(c), content_checksum=True)


def all_frames():
    return {"seven": seven(False), "seven_sums": seven(True), "plain": plain_oracle(), "sized": sized_oracle(),
            "sums_sized": write_frame(seven_pieces()[:3] + seven_pieces()[5:], block_checksums=True, content_checksum=True,
                                      with_content_size=True)}


# ---- frames that are not sound: what lz4flex_frame_index_create must answer is what the oracle's frame_decompress answers
def too_big_block():
    """a valid block that decodes to block size + 1 bytes"""
    return O.compress(text()[:BLOCK + 1])


def offset_zero_block():
    """literals "abcd", then a match with offset 0"""
    return bytes([0x40]) + b"abcd" + bytes([0, 0]) + bytes([0x50]) + b"vwxyz"


def broken_frames():
    w = seven(False)
    t = text()
    out = {"cut 9 bytes short": w.frame[:-9]}
    f = bytearray(w.frame)
    struct.pack_into("<I", f, w.payload_off[5] - 4, BLOCK + 1)
    out["BlockInfo above the block size"] = bytes(f)
    out["a block of block size + 1 bytes"] = write_frame(seven_pieces(), payloads={5: (too_big_block(), False)}).frame
    out["offset 0 in the first sequence"] = write_frame(seven_pieces(), payloads={1: (offset_zero_block(), False)}).frame
    # (stream order: a bad block in front of a BlockInfo that is too big wins; behind it, it is never reached)
    f = bytearray(write_frame(seven_pieces(), payloads={1: (offset_zero_block(), False)}).frame)
    struct.pack_into("<I", f, write_frame(seven_pieces(), payloads={1: (offset_zero_block(), False)}).payload_off[5] - 4, BLOCK + 1)
    out["offset 0 in front of a BlockInfo above the block size"] = bytes(f)
    good = write_frame([t[:3000], t[:500]], with_content_size=True)
    f = bytearray(good.frame)
    struct.pack_into("<Q", f, 6, 3501)
    f[14] = (O.xxh32(bytes(f[4:14])) >> 8) & 0xFF
    out["a wrong content size"] = bytes(f)
    out["a skippable frame first"] = struct.pack("<II", 0x184D2A53, 5) + b"12345" + w.frame
    out["wrong magic"] = b"\x05\x22\x4d\x18" + w.frame[4:]
    out["header checksum"] = w.frame[:6] + bytes([w.frame[6] ^ 1]) + w.frame[7:]
    out["cut inside the header"] = w.frame[:5]
    return out


def no_end_mark():
    """the frame ends where a BlockInfo word would start: the reference's reader returns what it has and leaves the frame open
    (src/frame/decompress.rs:231-238); an index is not made of it (-LZ4FLEX_FE_IO, the walk's "truncated")"""
    return seven(False).frame[:-4]
