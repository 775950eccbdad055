"""Blocks for lz4flex_decompress_batch_ex's prefix / chained / dictionary modes: written with lz4_writer.Writer to sit on the decoders'
boundaries, or cut out of the oracle's Linked frames.  Shared by the CPU tests (test_decompress_ext_oracle.py: the writer, the oracle's
prefix and dictionary decoders and its frame decoder agree on every block) and the GPU tests (test_gpu_decompress_ext.py), so the GPU
tests use only blocks whose meaning the CPU suite has pinned."""
import random
import struct

from lz4_writer import Writer

# 0 ... 17 bytes (the sequence decoder's 16-byte reload alignment), its 1 280-byte KEEP and 3 584-byte window, 64 KiB (what a match can
# reach) and a prefix of which only the last 64 KiB are reachable
PREFIX_LENS = (0, 1, 3, 4, 15, 16, 17, 1279, 1280, 1281, 3583, 3584, 3585, 65535, 65536, 65537, 200000)
# offsets on both sides of the sequence decoder's KEEP / window (1 280 / 3 584) and of the workgroup decoder's windows and tiles (test
# geometry: 512 + 1 024-byte window, 2 KiB tiles; production: larger powers of two)
WINDOW_OFFSETS = (63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1279, 1280, 1281, 1535, 1536, 1537, 2047, 2048, 2049, 3583, 3584,
                  3585, 4095, 4096, 4097, 8192, 16383, 16384, 32768, 49152, 65535)


def prefix_bytes(n, seed=0):
    """compressible, not periodic: words drawn from a small vocabulary, so blocks behind it find matches at every distance"""
    rnd = random.Random(seed * 7919 + n)
    words = [bytes(rnd.getrandbits(8) for _ in range(rnd.randint(2, 9))) for _ in range(64)]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words)
    return bytes(out[:n])


def writer_blocks(prefix, seed=0):
    """[(name, block, new bytes or None)] for a sink that holds `prefix`: None = an invalid block (the oracle says what it is)"""
    p = len(prefix)
    rnd = random.Random(seed * 1000003 + p)
    out = []

    def W(k):
        return Writer(seed * 100 + k, prefix)

    def add(name, w, tail=5):
        c, new = w.end(tail)
        out.append(("%s [prefix %d]" % (name, p), c, new))

    def bad(name, w, tail=5):
        c, _ = w.end(tail)
        out.append(("%s [prefix %d]" % (name, p), c, None))

    reach = min(p, 65535)
    add("literals only", W(1), 20)
    add("empty block", W(2), 0)                                  # b"\x00": 0 new bytes, valid with no room behind the prefix
    if p >= 1:
        add("source = the prefix's first reachable byte", W(3).seq(0, reach, 4).seq(9, 9, 12))
        add("source = the prefix's first reachable byte, 40 bytes", W(4).seq(0, reach, 40))
        add("from the prefix into the new bytes", W(5).seq(0, min(p, 8), 30).seq(2, min(p + 2, 300), 600))
        add("offset 1 on the first byte", W(6).seq(0, 1, 100))
        add("offset 1 on the first byte, 20 000 bytes", W(7).seq(0, 1, 20000).seq(1, 3, 5))
        for per in (2, 3, 17, 100, 1000, 1023):
            if per <= p:
                add("period %d from the prefix" % per, W(8 + per).seq(0, per, 1500 + per))
    if p + 1 <= 65535:
        bad("offset one behind the prefix", W(20).bad_seq(0, p + 1, 4))
    if p + 6 <= 65535:
        bad("offset one behind the prefix, after literals", W(21).bad_seq(5, p + 6, 4))
    if p >= 1000:
        w = W(22)
        for ml in (4, 64, 300, 5000):
            w.seq(10, min(p + 10, 65535), ml)          # (every call: as far back as the format reaches, the source in the prefix)
        add("far matches", w)
    w = W(23)
    w.seq(32, 32, 8)
    for _ in range(3):
        for off in WINDOW_OFFSETS:
            lit = rnd.randint(0, 20)
            if off <= len(w.out) + lit:
                w.seq(lit, off, rnd.choice((4, 15, 16, 17, 33, 64, 300, 1100)))
    add("sources on both sides of the windows", w)
    w = W(24)
    w.seq(max(0, 4 - p), 1, 4)
    for _ in range(300):
        lit = rnd.randint(0, 20)
        w.seq(lit, rnd.randint(1, min(len(w.out) + lit, 65535)), rnd.choice((4, 5, 9, 19, 20, 100, 273, 1500)))
    add("mixed", w)
    return out


def big_block(prefix, size=1 << 20, seed=0):
    """a block of `size` new bytes behind `prefix` whose matches reach up to 64 KiB back: into the prefix only in its first 64 KiB"""
    rnd = random.Random(seed + 77)
    w = Writer(seed + 78, prefix)
    while len(w.out) - w.base < size:
        lit = rnd.randint(0, 30)
        w.seq(lit, rnd.randint(1, min(len(w.out) + lit, 65535)), rnd.randint(4, 300))
    return w.end(5)


def frame_blocks(frame):
    """the blocks of an LZ4 frame (src/frame/header.rs): [(compressed?, bytes)], and the frame's block size in bytes"""
    assert frame[:4] == b"\x04\x22\x4d\x18"
    flg, bd = frame[4], frame[5]
    pos = 6 + (8 if flg & 0x08 else 0) + (4 if flg & 0x01 else 0) + 1
    bsize = {4: 64 << 10, 5: 256 << 10, 6: 1 << 20, 7: 4 << 20}[(bd >> 4) & 7]
    out = []
    while True:
        (v,) = struct.unpack_from("<I", frame, pos)
        pos += 4
        if v == 0:
            break
        n = v & 0x7FFFFFFF
        out.append((not (v >> 31), frame[pos:pos + n]))
        pos += n + (4 if flg & 0x10 else 0)
    return out, bsize
