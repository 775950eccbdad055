"""GPU (-m gpu): the frame layer's calls at the shapes where a group of their descriptor columns is EMPTY (lz4_flex_amd/csrc/frame_cols.h:
a column of no elements shares its start with its neighbour and must never be touched) -- no compressed block, no stored block, no
checksum entry, no plain entry, no chain columns, no item slot, no head.

Three streams of three blocks each at BlockSize::Max64KB: two full blocks and a tail of 1 000 bytes.  Every case expects the original
bytes, and the same bytes from the oracle's FrameDecoder (lz4_flex's, restated), which is computed once per frame and left alone."""
import struct

import numpy as np
import pytest

import oracle_api as O

pytestmark = pytest.mark.gpu
BS = 65536
SIZE = 2 * BS + 1000
STORED = 0x80000000


@pytest.fixture(scope="module")
def fr():
    from lz4_flex_amd import _lib, frame
    assert _lib.load().lz4flex_device_count() >= 1
    return frame


@pytest.fixture(scope="module")
def streams():
    rng = np.random.default_rng(25)
    text = O.fixture_plain("compression_65k") + O.fixture_plain("compression_66k_JSON")
    return {"random": [rng.integers(0, 256, SIZE, dtype=np.uint8).tobytes() for _ in range(3)],
            "text": [(text[1000 * i:] + text)[:SIZE] for i in range(3)]}


def _block_words(frame, sums):
    """the BlockInfo words of a frame whose header is the 7 bytes without a content size"""
    at, words = 7, []
    while True:
        w = struct.unpack_from("<I", frame, at)[0]
        if w == 0:
            return words
        words.append(w)
        at += 4 + (w & ~STORED) + (4 if sums else 0)


def _reference_frames(ss, block_mode, sums):
    """frames of the oracle's FrameEncoder and what its FrameDecoder makes of them"""
    frames = []
    for s in ss:
        rc, f = O.frame_compress(s, block_mode=block_mode, block_size=4, block_checksums=sums, content_checksum=sums)
        assert rc == 0
        rc, back, used = O.frame_decompress(f, SIZE)
        assert rc == 0 and back == s and used == len(f)
        frames.append(f)
    return frames


@pytest.fixture(scope="module")
def frames(streams):
    out = {"a": _reference_frames(streams["random"], 0, False),       # every block stored, no checksum
           "b": _reference_frames(streams["text"], 0, True),          # no stored block, block and content checksums
           "c": _reference_frames(streams["text"], 1, False)}         # Linked
    assert all(len(w) == 3 and all(v & STORED for v in w) for w in (_block_words(f, False) for f in out["a"]))
    assert all(len(w) == 3 and not any(v & STORED for v in w) for w in (_block_words(f, True) for f in out["b"]))
    assert all(len(w) == 3 and not any(v & STORED for v in w) for w in (_block_words(f, False) for f in out["c"]))
    return out


@pytest.mark.parametrize("case", ["a stored only", "b compressed with checksums", "c linked only", "d independent and linked"])
def test_decompress_many(fr, streams, frames, case):
    if case[0] == "d":
        fs, want = [frames["b"][0], frames["c"][1]], [streams["text"][0], streams["text"][1]]
    else:
        fs, want = frames[case[0]], streams["random" if case[0] == "a" else "text"]
    assert fr.decompress_frames(fs, [SIZE] * len(fs)) == want
    assert fr.decompress_frames(fs, [SIZE + 70000] * len(fs)) == want


@pytest.mark.parametrize("block_mode", [0, 1])
@pytest.mark.parametrize("compress_mode", ["fast", "exact"])
@pytest.mark.parametrize("kind", ["random", "text"])
def test_compress_many(fr, streams, kind, compress_mode, block_mode):
    from lz4_flex_amd import block
    ss = streams[kind]
    info = fr.FrameInfo(block_mode=fr.BlockMode(block_mode), block_size=fr.BlockSize.Max64KB)
    block.set_compress_mode(compress_mode)
    try:
        got = fr.compress_frames(ss, info)
    finally:
        block.set_compress_mode("fast")
    for s, f in zip(ss, got):
        rc, back, used = O.frame_decompress(f, SIZE)
        assert rc == 0 and back == s and used == len(f)
        if compress_mode == "exact":
            rc, exp = O.frame_compress(s, block_mode=block_mode, block_size=4)
            assert rc == 0 and f == exp
    assert fr.decompress_frames(got, [SIZE] * 3) == ss


# (what the call is about, ranges): content offsets of the 3-block frame
RANGE_CALLS = [("no item slot", [(0, 0), (SIZE, 5), (SIZE + 10, 1), (70000, 0)]),
               ("no head", [(BS, 3000)]),
               ("one head", [(BS + 100, 3000)])]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("call", RANGE_CALLS, ids=[c[0].replace(" ", "_") for c in RANGE_CALLS])
def test_read_ranges(fr, streams, frames, call, which, device):
    import torch
    f, full = frames[which][0], streams["random" if which == "a" else "text"][0]
    src = torch.from_numpy(np.frombuffer(f, np.uint8).copy()).cuda() if device else f
    with fr.FrameIndex(src) as ix:
        assert (ix.blocks, ix.content_size, ix.frame_bytes) == (3, SIZE, len(f))
        assert ix.read_ranges(call[1]) == [full[o:o + n] for o, n in call[1]]
