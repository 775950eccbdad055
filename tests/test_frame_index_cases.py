"""CPU: the frames tests/frame_index_cases.py writes by hand are frames -- the oracle's FrameDecoder decodes each to its pieces -- and the
broken ones are broken the way their names say.  The GPU tests of the frame index then do not rest on the writer alone."""
import pytest

import frame_index_cases as FC
import oracle_api as O
import partial_model

FE_DECOMPRESSION, FE_IO, FE_WRONG_MAGIC, FE_BLOCK_TOO_BIG, FE_HEADER_CHECKSUM, FE_SKIPPABLE, FE_CONTENT_LENGTH = 17, 18, 21, 24, 25, 28, 30


@pytest.fixture(scope="module")
def frames():
    return FC.all_frames()


def test_the_oracle_decodes_every_written_frame_to_its_pieces(frames):
    for name, w in frames.items():
        rc, back, used = O.frame_decompress(w.frame, len(w.content) + 64)
        assert (rc, back, used) == (0, w.content, len(w.frame)), name
        po, lw, end = FC.walk(w.frame, w.block_checksums, w.payload_off[0] - 4)
        assert (po, lw) == (w.payload_off, w.len_word), name
        assert [b - a for a, b in zip(w.content_off, w.content_off[1:])] == [len(p) for p in w.pieces]
        for b, piece in enumerate(w.pieces):                    # every block alone is its piece
            pay = w.frame[w.payload_off[b]:w.payload_off[b] + (w.len_word[b] & ~FC.STORED)]
            assert (pay if w.len_word[b] & FC.STORED else O.decompress(pay, FC.BLOCK)[1]) == piece, (name, b)


def test_the_seven_block_frame_has_the_shapes_it_is_for():
    for sums in (False, True):
        w = FC.seven(sums)
        assert [len(p) for p in w.pieces] == [100, 65536, 1, 65536, 7, 65531, 40000] and w.stored == FC.SEVEN_STORED
        assert O.frame_decompress(w.frame[:-9], 1 << 20)[0] == FE_IO


def test_the_broken_frames_are_broken_as_named():
    got = {name: O.frame_decompress(f, 1 << 20)[:2] for name, f in FC.broken_frames().items()}
    assert got["cut 9 bytes short"][0] == FE_IO
    assert got["BlockInfo above the block size"][0] == FE_BLOCK_TOO_BIG
    assert got["a block of block size + 1 bytes"] == (FE_DECOMPRESSION, (FC.BLOCK + 1, FC.BLOCK, 1))          # OutputTooSmall
    assert got["offset 0 in the first sequence"][0] == FE_DECOMPRESSION and got["offset 0 in the first sequence"][1][2] == 4
    assert got["offset 0 in front of a BlockInfo above the block size"] == got["offset 0 in the first sequence"]
    assert got["a wrong content size"] == (FE_CONTENT_LENGTH, (3501, 3500, 0))
    assert got["a skippable frame first"][0] == FE_SKIPPABLE and got["a skippable frame first"][1][0] == 5
    assert got["wrong magic"][0] == FE_WRONG_MAGIC and got["header checksum"][0] == FE_HEADER_CHECKSUM
    assert got["cut inside the header"][0] == FE_IO
    assert O.frame_decompress(FC.no_end_mark(), 1 << 20)[:2] == (0, FC.seven().content)
    assert O.decompress(FC.too_big_block(), FC.BLOCK + 1)[0] == "ok"
    assert partial_model.partial(FC.offset_zero_block(), 5)[0] == 4
