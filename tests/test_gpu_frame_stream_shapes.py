"""GPU tests (-m gpu) that pin what the streaming FrameEncoder / FrameDecoder and the two one-shot calls do with the SHAPE of the calls:
write sizes, flushes, batch sizes and frames on one encoder; read sizes, fill_buf / consume and batch sizes on the decoder.  64 KiB
blocks throughout, no stream above 1 MiB.

Encoder: in compress_mode exact the frame is the oracle's FrameEncoder's, byte for byte, for the same writes and flushes
(`O.frame_compress(data, chunks, flush=True)`: a flush() behind every chunk); in compress_mode fast (the throughput encoder: its own
parse) the oracle's FrameDecoder returns the data and consumes the whole frame, and every block decodes to as many bytes as the
oracle's block at that place.

Decoder: frames of the oracle's encoder and frames written block by block (tests/frame_index_cases.py), each drained with read(7),
read(65536), read(1 MiB), read(3 MiB) (the last two: decoded straight into the reader's buffer), fill_buf / consume and the one-shot
call, under automatic batches and batches of one and of three blocks.  The bytes are the content; a read returns 0 exactly once
behind every block that decodes to nothing and once at the end of the frame, with every byte in front of it delivered
(src/frame/decompress.rs:344-349).  (The one-shot call has no batch setting: it runs once per frame and capacity.)  Errors are
tests/test_gpu_frame_damage.py's subject."""
import functools
import io
import struct

import numpy as np
import pytest

import frame_index_cases as FC
import oracle_api as O

pytestmark = pytest.mark.gpu

BS = 65536
STORED = 0x80000000
LINKED_CHUNKS = [65536, 65536, 65536, 1000, 65536, 30000, 65536, 65536]


@pytest.fixture(scope="module")
def fr():
    from lz4_flex_amd import _lib, frame
    assert _lib.load().lz4flex_device_count() >= 1
    return frame


@functools.lru_cache(maxsize=None)
def content():
    """7 blocks and 1 000 bytes: JSON, JSON, random (a stored block), text, JSON that repeats what is in front of it"""
    t, r = FC.text(), FC.rand()
    text = O.fixture_plain("compression_65k")
    out = t[:2 * BS] + r + (text + text)[:BS] + t[300:300 + 3 * BS + 1000]
    assert len(out) == 7 * BS + 1000
    return out


# ---------------------------------------------------------------------------------------------------------------- encoder
# (name, content length, batch bytes or None, ops): ops are write sizes, "flush" and "finish" (try_finish: the next write opens a new
# frame); what is left of the content behind the last op is written in one write, and the encoder finished
PATTERNS = [
    ("one write", 5 * BS + 1000, None, []),
    ("writes of 1000", 5 * BS + 1000, None, [1000] * 328),
    ("one batch exactly", 2 * BS, 2 * BS, []),
    ("two batches and 5000", 4 * BS + 5000, 2 * BS, []),
    ("1000 then 70000", 71000, 2 * BS, [1000]),
    ("1000 then 140000", 141000, 2 * BS, [1000]),                       # staged, then the stage is full, then the rest
    ("flush after 1000 and 71000", 5 * BS + 1000, None, [1000, "flush", 70000, "flush"]),
    ("flush after 1000 and 71000, batches", 5 * BS + 1000, 2 * BS, [1000, "flush", 70000, "flush"]),
    ("flush with nothing pending", 3 * BS + 1000, None, ["flush", 3 * BS + 1000, "flush", "flush"]),
    ("two frames", 5 * BS + 1000, None, [2 * BS + 500, "finish"]),
    ("two frames, short first", 3 * BS, 2 * BS, [1000, "finish"]),
]
MODES = [("independent-exact", 0, "exact"), ("independent-fast", 0, "fast"), ("linked-fast", 1, "fast"), ("linked-exact", 1, "exact")]


def run_pattern(fr, data, block_mode, batch, ops):
    """-> (the bytes written, [(frame's content, its chunks: the write sizes in front of each flush)])"""
    buf = io.BytesIO()
    e = fr.FrameEncoder.with_frame_info(fr.FrameInfo(block_size=fr.BlockSize.Max64KB, block_mode=fr.BlockMode(block_mode)), buf)
    if batch:
        e.set_batch_bytes(batch)
    frames, at, start, chunks, since = [], 0, 0, [], 0
    for op in list(ops) + [len(data) - sum(o for o in ops if isinstance(o, int)), "finish"]:
        if op == "flush":
            e.flush()
            if since:
                chunks.append(since)
            since = 0
        elif op == "finish":
            e.try_finish()
            frames.append((data[start:at], chunks + ([since] if since else [])))
            start, chunks, since = at, [], 0
        elif op:
            assert e.write(data[at:at + op]) == op
            at += op; since += op
    assert at == len(data)
    return buf.getvalue(), frames


def block_lengths(frame, linked):
    """(decoded length of every block, the content, the frame's length): BlockInfo words, stored blocks as they are, compressed ones
    through the oracle's block decoder (a Linked frame's with the 64 KiB in front of them in its sink)"""
    lens, out, p = [], b"", 7
    while True:
        (w,) = struct.unpack_from("<I", frame, p)
        p += 4
        if w == 0:
            return lens, out, p
        n = w & ~STORED
        pay = frame[p:p + n]
        p += n
        if w & STORED:
            piece = pay
        else:
            prefix = out[-65536:] if linked else b""
            rc, piece = O.decompress_prefix(pay, prefix, len(prefix) + BS)
            assert rc == "ok", (rc, piece)
        lens.append(len(piece)); out += piece


def oracle_frame(data, chunks, block_mode):
    rc, f = O.frame_compress(data, chunks=chunks, flush=True, block_size=4, block_mode=block_mode)
    assert rc == 0
    return f


def check_frames(written, frames, block_mode, exact):
    at = 0
    for data, chunks in frames:
        want = oracle_frame(data, chunks, block_mode)
        want_lens, want_data, want_end = block_lengths(want, block_mode == 1)
        assert want_data == data and want_end == len(want)
        if exact:
            assert written[at:at + len(want)] == want
            at += len(want)
            continue
        rc, back, used = O.frame_decompress(written[at:], len(data))
        assert rc == 0 and back == data
        lens, got, end = block_lengths(written[at:], block_mode == 1)
        assert got == data and end == used
        assert lens == want_lens
        at += used
    assert at == len(written)


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("pattern", PATTERNS, ids=[p[0] for p in PATTERNS])
def test_encoder_write_patterns(fr, pattern, mode):
    from lz4_flex_amd import block
    _, size, batch, ops = pattern
    _, block_mode, compress_mode = mode
    data = content()[:size]
    block.set_compress_mode(compress_mode)
    try:
        written, frames = run_pattern(fr, data, block_mode, batch, ops)
    finally:
        block.set_compress_mode("fast")
    assert len(frames) == 1 + ops.count("finish")
    check_frames(written, frames, block_mode, compress_mode == "exact")


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("size", [0, 1000, BS, 5 * BS + 1000])
def test_encoder_one_shot(fr, size, mode):
    from lz4_flex_amd import block
    _, block_mode, compress_mode = mode
    data = content()[:size]
    block.set_compress_mode(compress_mode)
    try:
        f = fr.compress_frame(data, fr.FrameInfo(block_size=fr.BlockSize.Max64KB, block_mode=fr.BlockMode(block_mode)))
    finally:
        block.set_compress_mode("fast")
    check_frames(f, [(data, [size] if size else [])], block_mode, compress_mode == "exact")


def test_flushed_oracle_frames_have_short_blocks():
    """what the expectations above rest on: the oracle's flushed frames hold the blocks the chunks say"""
    for mode in (0, 1):
        lens, data, _ = block_lengths(oracle_frame(content()[:sum(LINKED_CHUNKS)], LINKED_CHUNKS, mode), mode == 1)
        assert lens == LINKED_CHUNKS and data == content()[:sum(LINKED_CHUNKS)]
        lens, _, _ = block_lengths(oracle_frame(content()[:141000], [1000, 140000], mode), mode == 1)
        assert lens == [1000, BS, BS, 140000 - 2 * BS]


# ---------------------------------------------------------------------------------------------------------------- decoder
def as_linked(w):
    """the same blocks behind a Linked header (a block that refers to nothing in front of it is a Linked frame's block too)"""
    return FC.Written(FC.header(w.content, block_size=4, block_mode=1) + w.frame[7:], w.pieces, w.content_off, w.payload_off, w.len_word, False)


@functools.lru_cache(maxsize=None)
def frames():
    """name -> (frame, pieces: the content block by block)"""
    c, t, r = content(), FC.text(), FC.rand()
    ind = FC.oracle_frame(c[:5 * BS + 1000], block_size=4)
    assert len(ind.pieces) == 6 and len(ind.pieces[-1]) == 1000
    n = sum(LINKED_CHUNKS)
    lnk = oracle_frame(c[:n], LINKED_CHUNKS, 1)
    cuts = np.cumsum([0] + LINKED_CHUNKS)
    out = {"independent": (ind.frame, ind.pieces), "linked": (lnk, [c[a:b] for a, b in zip(cuts[:-1], cuts[1:])])}
    stored =FC.write_frame([t[:BS], t[:3000], r[:5000], t[100:BS + 100], r, t[:2000]])
    assert stored.stored == [False, False, True, False, True, False]
    mid = FC.write_frame([t[:BS], t[:3000], b"", t[7:4007], r[:300]], payloads={2: (b"\x00", False)})
    first = FC.write_frame([t[:BS], t[:3000], t[50:BS + 50], b"", t[7:4007], b"", r[:300]], payloads={3: (b"\x00", False), 5: (b"\x00", False)})
    for name, w in (("stored", stored), ("empty middle", mid), ("empty first of a batch", first)):
        out[name] = (w.frame, w.pieces)
        out[name + ", linked"] = (as_linked(w).frame, w.pieces)
    return out


FRAME_NAMES = ["independent", "linked", "stored", "stored, linked", "empty middle", "empty middle, linked", "empty first of a batch",
               "empty first of a batch, linked"]
BATCHES = [None, BS, 3 * BS]


def expected_zeros(pieces):
    """the number of bytes delivered at each read that returns 0: behind every empty block, and at the end of the frame"""
    at, out = 0, []
    for p in pieces:
        at += len(p)
        if not p:
            out.append(at)
    return out + [at]


def drain_read(d, n, want_zeros):
    out, zeros = [], []
    got = 0
    while len(zeros) < want_zeros:
        b = d.read(n)
        assert len(b) <= n
        if b:
            out.append(b); got += len(b)
        else:
            zeros.append(got)
    return b"".join(out), zeros


def drain_fill_buf(d, want_zeros):
    out, zeros = [], []
    got = 0
    while len(zeros) < want_zeros:
        b = d.fill_buf()
        if not b:
            zeros.append(got)
            continue
        assert d.fill_buf() == b                       # nothing consumed: the same bytes again
        k = min(len(b), 50000)
        out.append(b[:k]); got += k
        d.consume(k)
    return b"".join(out), zeros


@pytest.mark.parametrize("batch", BATCHES, ids=["auto", "1 block", "3 blocks"])
@pytest.mark.parametrize("way", ["read 7", "read 65536", "read 1 MiB", "read 3 MiB", "fill_buf"])
@pytest.mark.parametrize("name", FRAME_NAMES)
def test_decoder_drains(fr, name, way, batch):
    frame, pieces = frames()[name]
    want, zeros = b"".join(pieces), expected_zeros(pieces)
    d = fr.FrameDecoder.new(io.BytesIO(frame))
    if batch:
        d.set_batch_bytes(batch)
    if way == "fill_buf":
        got, at = drain_fill_buf(d, len(zeros))
    else:
        got, at = drain_read(d, {"read 7": 7, "read 65536": 65536, "read 1 MiB": 1 << 20, "read 3 MiB": 3 << 20}[way], len(zeros))
    assert got == want
    assert at == zeros
    assert d.read(65536) == b"" and d.fill_buf() == b""      # no second frame: EOF


@pytest.mark.parametrize("roomy", [False, True], ids=["exact capacity", "2 MiB"])
@pytest.mark.parametrize("name", FRAME_NAMES)
def test_decoder_one_shot(fr, name, roomy):
    frame, pieces = frames()[name]
    cap = 2 << 20 if roomy else len(b"".join(pieces))
    rc, want, want_used = O.frame_decompress(frame, cap)
    assert rc == 0 and want == b"".join(pieces)[:expected_zeros(pieces)[0]]     # the reader stops at the first read that returns 0
    got, used = fr.decompress_frame(frame, cap)
    assert got == want and used == want_used
