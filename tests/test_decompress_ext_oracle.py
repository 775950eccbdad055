"""CPU: the checker of tests/test_gpu_decompress_ext.py.  Its blocks (tests/ext_cases.py) mean what the writer says they mean, the
oracle's prefix decoder (decompress_internal with a sink position) agrees with its dictionary decoder on the new bytes, and decoding
the oracle's own Linked frames block by block behind their prefixes gives the oracle's frame decoder's result."""
import pytest

import ext_cases as X
import oracle_api as O


@pytest.mark.parametrize("p", X.PREFIX_LENS)
def test_writer_blocks_equal_the_oracle(p):
    prefix = X.prefix_bytes(p)
    blocks = X.writer_blocks(prefix)
    assert len(blocks) >= 4
    for name, c, new in blocks:
        got = O.decompress_prefix(c, prefix, p + 65536 + len(c) * 255)
        if new is None:
            assert got[0] == "OffsetOutOfBounds", (name, got[0])
            continue
        assert got == ("ok", new), name
        assert O.decompress_prefix(c, prefix, p + len(new)) == ("ok", new), name                  # an exact sink
        if new:
            st, det = O.decompress_prefix(c, prefix, p + len(new) - 1)
            assert st == "OutputTooSmall" and det[1] == p + len(new) - 1 and det[0] > det[1], (name, st, det)   # absolute detail
        # prefix and dictionary decoding agree: the prefix's last 64 KiB as an external dictionary, an empty sink
        assert O.decompress(c, len(new), dict_data=prefix[-65536:] if p else None) == ("ok", new), name


def test_big_block_behind_a_prefix():
    prefix = X.prefix_bytes(65536, 1)
    c, new = X.big_block(prefix)
    assert len(new) >= 1 << 20
    assert O.decompress_prefix(c, prefix, 65536 + len(new)) == ("ok", new)
    assert O.decompress(c, len(new), dict_data=prefix) == ("ok", new)
    assert O.decompress(c, len(new))[0] == "OffsetOutOfBounds"          # it does reach into the prefix


def test_prefix_refuses_a_sink_shorter_than_the_prefix():
    with pytest.raises(ValueError):
        O.decompress_prefix(b"\x00", b"abc", 2)
    assert O.decompress_prefix(b"\x00", b"abc", 3) == ("ok", b"")
    assert O.decompress_prefix(b"\x10x", b"abc", 3) == ("OutputTooSmall", (4, 3))


def test_prefix_with_a_dictionary():
    """both at once (lz4flex_decompress_batch_ex allows it for the reference-order kernel): offsets beyond the prefix reach the
    dictionary, whose end lies right before the prefix's start"""
    prefix, d = b"0123456789", b"abcdefghij"
    blk = bytes([0x00 | 0, 12, 0]) + bytes([0x50]) + b"vwxyz"   # match: offset 12 (2 bytes into the dict's tail), 4 bytes
    st, new = O.decompress_prefix(blk, prefix, 100, dict_data=d)
    assert (st, new) == ("ok", b"ij01vwxyz")
    assert O.decompress_prefix(bytes([0x00, 21, 0, 0x50]) + b"vwxyz", prefix, 100, dict_data=d)[0] == "OffsetOutOfBounds"
    assert O.decompress_prefix(bytes([0x00, 20, 0, 0x50]) + b"vwxyz", prefix, 100, dict_data=d) == ("ok", b"abcdvwxyz")


@pytest.mark.parametrize("bs", (4, 5))
def test_linked_frames_block_by_block(bs):
    """block k of a Linked frame decoded behind the frame's earlier output == the frame decoder; the last block is short"""
    plain = (O.fixture_plain("compression_66k_JSON") + O.fixture_plain("compression_65k")) * 5
    plain = plain[:len(plain) - 12345]
    rc, fr = O.frame_compress(plain, block_size=bs, block_mode=1)
    assert rc == 0
    blocks, bsize = X.frame_blocks(fr)
    assert len(blocks) >= 3 and len(plain) % bsize != 0
    out = b""
    reached = False
    for compressed, data in blocks:
        if not compressed:
            out += data
            continue
        st, new = O.decompress_prefix(data, out, len(out) + bsize)
        assert st == "ok", st
        if out:
            reached |= O.decompress(data, bsize)[0] != "ok"     # (some block needs its prefix)
        out += new
    assert reached
    assert O.frame_decompress(fr, len(plain) + 16)[:2] == (0, out) and out == plain
