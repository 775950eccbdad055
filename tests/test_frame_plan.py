"""lz4_flex_amd/csrc/frame_plan.h on the CPU: block sizes, the table mode of an Independent frame's blocks and the window of a
Linked frame's, walked past the table reposition near 2 GiB that no test reaches through the API (it takes more than 2 GiB of data).

The expected values never come from the header: `OracleEncoder` is the oracle's `enc_write_block` (oracle/lz4flex_frame.c:206-256,
the reference's src/frame/compress.rs:261-371) restated on lengths alone, with its own field names, in the coordinates of ITS src
buffer; `pos0` / `dict_pos` say where src[0] and ext_dict[0] lie in the stream.  Full blocks are also held against
`sharded.block_flags`, the Python statement the sharded path already uses.

The shim's `skip` restates the replay of sharded.cpp (`first_block` full blocks, then the rank's own): it proves `TableOffset` under
that replay, not sharded.cpp's own loop, which tests/test_gpu_sharded_native.py runs at small `first_block`."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lz4_flex_amd import sharded as S  # noqa: E402

SRC = os.path.join(ROOT, "tests", "sim", "frame_plan_shim.cpp")
HDR = os.path.join(ROOT, "lz4_flex_amd", "csrc", "frame_plan.h")
SO = os.path.join(ROOT, "tests", "sim", "libframe_plan_shim.so")

WINDOW = 65536
FIRST, CONT = 2, 3                       # LZ4FLEX_BLOCK_FRAME_FIRST / _CONTINUATION (include/lz4flex_amd.h)
SIZES = {4: 64 << 10, 5: 256 << 10, 6: 1 << 20, 7: 4 << 20}
# so + bs + 65536 >= 0x7FFFFFFF with so = k * bs: the first k for which it holds is the first block that is FIRST again
REPOSITION_INDEX = {64 << 10: 32766, 256 << 10: 8191, 1 << 20: 2047, 4 << 20: 511}

_m = None


def shim():
    global _m
    if _m is None:
        if not os.path.exists(SO) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(SO):
            subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-Wall", SRC, "-o", SO])
        m = C.CDLL(SO)
        u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
        m.fp_block_size_bytes.restype = C.c_uint64
        m.fp_block_size_bytes.argtypes = [C.c_int]
        m.fp_block_size_from_buf_length.restype = C.c_int
        m.fp_block_size_from_buf_length.argtypes = [C.c_uint64]
        for name in ("fp_stream_max", "fp_window_size"):
            getattr(m, name).restype = C.c_uint64
        m.fp_uncompressed_bit.restype = C.c_uint32
        m.fp_table_modes.restype = None
        m.fp_table_modes.argtypes = [C.c_uint64, C.c_uint64, u64p, C.c_uint64, u32p]
        m.fp_linked_walk.restype = None
        m.fp_linked_walk.argtypes = [C.c_uint64, C.c_uint64, u64p, C.c_uint64, u64p, u64p]
        for name, n_args in (("fp_blocks_per_launch", 3), ("fp_decode_slot_cap", 2), ("fp_launch_out_budget", 3), ("fp_pos_blocks", 2)):
            getattr(m, name).restype = C.c_uint64
            getattr(m, name).argtypes = [C.c_uint64, C.c_uint64] + [C.c_int] * (n_args - 2)
        m.fp_decode_ring_walk.restype = None
        m.fp_decode_ring_walk.argtypes = [C.c_uint64, u64p, C.c_uint64, u64p]
        m.fp_decode_ring_too_small.restype = None
        m.fp_decode_ring_too_small.argtypes = [C.c_uint64] * 7 + [u64p]
        m.fp_decode_runs.restype = C.c_uint64
        m.fp_decode_runs.argtypes = [C.c_uint64, C.POINTER(C.c_uint8), C.c_uint64, u64p, C.c_uint64]
        _m = m
    return _m


def table_modes(bs, lens, skip=0):
    lens = np.ascontiguousarray(lens, dtype=np.uint64)
    out = np.zeros(len(lens), dtype=np.uint32)
    shim().fp_table_modes(bs, skip, lens.ctypes.data_as(C.POINTER(C.c_uint64)), len(lens), out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return out


def linked_walk(bs, lens, pos=0):
    """(n, 8) in_off, dict_off, in_len, in_pos, dict_len, so, repos, flags; (n,) keep_from"""
    lens = np.ascontiguousarray(lens, dtype=np.uint64)
    out = np.zeros((len(lens), 8), dtype=np.uint64)
    keep = np.zeros(len(lens), dtype=np.uint64)
    p = C.POINTER(C.c_uint64)
    shim().fp_linked_walk(bs, pos, lens.ctypes.data_as(p), len(lens), out.ctypes.data_as(p), keep.ctypes.data_as(p))
    return out, keep


class OracleEncoder:
    """enc_write_block on lengths: every write is at most one block, so src_start == src_end between blocks"""

    def __init__(self, bs, linked, pos=0):
        self.bs, self.linked = bs, linked
        self.src_start = self.src_end = self.ext_dict_offset = self.ext_dict_len = self.src_stream_offset = 0
        self.pos0 = pos          # stream position of src[0]
        self.dict_pos = 0        # stream position of src[ext_dict_offset] as it was when the dictionary was set aside

    def write_block(self, n):
        """-> (table mode, in_off, dict_off, in_len, in_pos, dict_len, so, repos)"""
        assert 0 < n <= self.bs
        self.src_end += n                                                        # enc_write: vec_copy_overwriting
        repos = 0
        if self.src_stream_offset + self.bs + WINDOW >= 0xFFFFFFFF // 2:         # :266-271
            repos = self.src_stream_offset - self.ext_dict_len
            self.src_stream_offset = self.ext_dict_len
        mode = FIRST if self.src_stream_offset == 0 else CONT
        rec = (mode, self.pos0, self.dict_pos if self.ext_dict_len else 0, self.src_end, self.src_start, self.ext_dict_len,
               self.src_stream_offset, repos)
        src_len = self.src_end - self.src_start
        self.src_start += src_len
        if self.linked:                                                          # :327-356
            if self.src_start >= self.bs + WINDOW:
                self.ext_dict_offset = self.src_end - WINDOW
                self.dict_pos = self.pos0 + self.ext_dict_offset
                self.ext_dict_len = WINDOW
                self.src_stream_offset += self.src_end
                self.pos0 += self.src_end
                self.src_start = self.src_end = 0
            elif self.src_start + self.ext_dict_len > WINDOW:
                delta = min(self.ext_dict_len, self.src_start + self.ext_dict_len - WINDOW)
                self.ext_dict_offset += delta
                self.dict_pos += delta
                self.ext_dict_len -= delta
        else:                                                                    # :357-367
            self.pos0 += self.src_end
            self.src_start = self.src_end = 0
            self.src_stream_offset += src_len
        return rec


def mixed_lengths(rng, bs, n):
    """full blocks with short ones between them (flush() boundaries): 1 byte, around the window, one short of full"""
    short = [1, 2, 100, WINDOW - 1, WINDOW, WINDOW + 1, bs // 2, bs - 1]
    return [bs if rng.random() < 0.6 else min(bs, rng.choice(short + [rng.randrange(1, bs + 1)])) for _ in range(n)]


def test_block_sizes():
    m = shim()
    want = {4: 64 * 1024, 5: 256 * 1024, 6: 1024 * 1024, 7: 4 * 1024 * 1024, 8: 8 * 1024 * 1024}      # header.rs:68-77
    for code in range(9):
        assert m.fp_block_size_bytes(code) == want.get(code, 0), code
    for at, below, above in ((64 * 1024, 4, 5), (256 * 1024, 5, 7)):                                  # header.rs:57-67
        assert [m.fp_block_size_from_buf_length(at + d) for d in (-1, 0, 1)] == [below, below, above]
    assert m.fp_window_size() == WINDOW and m.fp_uncompressed_bit() == 0x80000000


@pytest.mark.parametrize("bs", sorted(SIZES.values()))
def test_table_mode_full_blocks(bs):
    at = REPOSITION_INDEX[bs]
    assert (at - 1) * bs + bs + WINDOW < 0x7FFFFFFF <= at * bs + bs + WINDOW       # the rule, by hand
    n = 2 * at + 3
    want = S.block_flags(0, n, bs)
    got = table_modes(bs, [bs] * n)
    assert np.array_equal(got, want)
    assert [i for i in range(n) if got[i] == FIRST] == [0, at, 2 * at]
    enc = OracleEncoder(bs, linked=False)
    assert [enc.write_block(bs)[0] for _ in range(n)] == list(want)                # (the restatement agrees with sharded.py)
    for first in (at - 1, at, at + 1, 2 * at - 1, 2 * at, 2 * at + 1):             # sharded.cpp: first_block full blocks, then its own
        assert np.array_equal(table_modes(bs, [bs] * 3, skip=first), S.block_flags(first, 3, bs)), first
        assert np.array_equal(table_modes(bs, [bs, bs, 1], skip=first), S.block_flags(first, 3, bs)), first


@pytest.mark.parametrize("bs", sorted(SIZES.values()))
def test_table_mode_short_blocks(bs):
    rng = random.Random(bs)
    # a short block in the middle: the offset moves by its length, so the reposition comes one block later than with full ones
    at = REPOSITION_INDEX[bs]
    lens = [bs] * (at + 2)
    lens[at // 2] = 1
    got = table_modes(bs, lens)
    assert [i for i in range(len(lens)) if got[i] == FIRST] == [0, at + 1]
    for _ in range(8):
        lens = mixed_lengths(rng, bs, 2 * at + rng.randrange(50))    # (about 0.65 block sizes per block: past the first reposition)
        enc = OracleEncoder(bs, linked=False)
        want = [enc.write_block(n)[0] for n in lens]
        assert list(table_modes(bs, lens)) == want
        assert want.count(FIRST) >= 2


def check_linked(bs, lens, pos=0):
    got, keep = linked_walk(bs, lens, pos)
    enc = OracleEncoder(bs, linked=True, pos=pos)
    before = 0                                         # bytes of the frame in front of the block
    n_repos = 0
    for i, n in enumerate(lens):
        want = enc.write_block(n)[1:]
        in_off, dict_off, in_len, in_pos, dict_len, so, repos, flags = (int(v) for v in got[i])
        assert (in_off, dict_off, in_len, in_pos, dict_len, so, repos) == want, (i, n)
        assert flags == 0
        assert dict_len <= WINDOW
        assert dict_len == 0 or dict_off + dict_len == in_off
        assert in_len <= 2 * bs + WINDOW
        assert in_pos + dict_len >= min(WINDOW, before)
        assert in_off + in_pos == pos + before         # the block is where the stream says it is
        assert in_len - in_pos == n
        before += n
        # what the next blocks can reach: the prefix and, while there is one, the dictionary in front of it
        assert int(keep[i]) == (min(enc.pos0, enc.dict_pos) if enc.ext_dict_len else enc.pos0)
        n_repos += repos != 0
    return n_repos


@pytest.mark.parametrize("bs", sorted(SIZES.values()))
def test_linked_window_random_lengths(bs):
    rng = random.Random(1000 + bs)
    for k in range(200):
        lens = mixed_lengths(rng, bs, rng.randrange(1, 24))
        check_linked(bs, lens, pos=0 if k % 2 else rng.randrange(1 << 40))       # (reset(pos): a later frame on one encoder)


def test_linked_window_beyond_4_gib():
    bs = 4 << 20
    assert check_linked(bs, [bs] * 1100) >= 2
    rng = random.Random(7)
    lens = [bs if rng.random() < 0.9 else rng.randrange(1, bs) for _ in range(1250)]
    assert sum(lens) > 1 << 32
    assert check_linked(bs, lens) >= 2


@pytest.mark.parametrize("bs", sorted(SIZES.values()))
def test_stream_max_never_repositions(bs):
    """what frame_many.cpp relies on for the streams it lays out in one go: a stream of STREAM_MAX bytes"""
    stream_max = shim().fp_stream_max()
    assert stream_max == 0x7FFF0000 - (8 << 20)
    lens = [bs] * (stream_max // bs) + ([stream_max % bs] if stream_max % bs else [])
    assert sum(lens) == stream_max
    modes = table_modes(bs, lens)
    assert modes[0] == FIRST and (modes[1:] == CONT).all()
    got, _ = linked_walk(bs, lens)
    assert not got[:, 6].any()                         # repos
    assert int(got[:, 5].max()) < 1 << 31              # so


# ---- the decoder's rules -----------------------------------------------------------------------------------------------------------
class OracleRing:
    """the oracle's decoder ring (oracle/lz4flex_frame.c, lz4o_frame_decompress; the reference's src/frame/decompress.rs:195-222, :280-306)
    on lengths alone: a buffer of two block sizes and a window, the reader takes every block before the next one is decoded"""

    def __init__(self, bs):
        self.bs, self.size = bs, 2 * bs + WINDOW
        self.dict_at = self.dict_n = self.at = 0

    def block(self, produced):
        """-> (sink end, dict_at, dict_n, at) as the block finds them"""
        if self.at + self.bs > self.size:                                      # :202-210
            self.dict_at, self.dict_n, self.at = self.at - WINDOW, WINDOW, 0
        elif self.at + self.dict_n > WINDOW:                                   # :211-221
            delta = min(self.dict_n, self.at + self.dict_n - WINDOW)
            self.dict_at += delta
            self.dict_n -= delta
        sink_end = self.dict_at if self.dict_n else self.at + self.bs          # :280-306: dst[..ext_dict_offset] / dst[..dst_start + bs]
        rec = (sink_end, self.dict_at, self.dict_n, self.at)
        self.at += produced
        return rec


def ring_walk(bs, lens):
    lens = np.ascontiguousarray(lens, dtype=np.uint64)
    out = np.zeros((len(lens), 5), dtype=np.uint64)
    p = C.POINTER(C.c_uint64)
    shim().fp_decode_ring_walk(bs, lens.ctypes.data_as(p), len(lens), out.ctypes.data_as(p))
    return out


@pytest.mark.parametrize("bs", sorted(SIZES.values()))
def test_decode_ring_random_blocks(bs):
    rng = random.Random(2600 + bs)
    for _ in range(20):
        lens = [bs if rng.random() < 0.6 else rng.choice([0, 0, 1, 100, WINDOW - 1, WINDOW, WINDOW + 1, bs // 2, bs - 1, rng.randrange(bs + 1)])
                for _ in range(400)]
        lens = [min(n, bs) for n in lens]
        ring = OracleRing(bs)
        got = ring_walk(bs, lens)
        wraps = 0
        for i, n in enumerate(lens):
            want = ring.block(n)
            assert tuple(int(v) for v in got[i][:4]) == want, (i, n)
            assert int(got[i][4]) == want[0] - want[3]
            assert bs <= want[0] - want[3] <= 2 * bs          # a block always fits; the ring never gives more than two
            wraps += i > 0 and want[3] == 0
        assert wraps >= 5
        assert max(int(r[4]) for r in got) > bs               # ... and right behind a wrap it does give more than one


def test_decode_ring_too_small():
    """(expected, actual) of a block whose sink started at `pos` of the launch's buffer become positions of the reference's sink:
    the distance from the block's start carried over to ring_start, and where the ring's sink ends"""
    m, out = shim(), (C.c_uint64 * 2)()
    bs = 65536
    m.fp_decode_ring_too_small(bs, 0, 0, 1000, 70000, 70000 + bs + 1, 70000 + bs, out)           # no dictionary: a block size behind ring_start
    assert list(out) == [1000 + bs + 1, 1000 + bs]
    m.fp_decode_ring_too_small(bs, 2 * bs, WINDOW, 0, 65536 + 3 * bs, 65536 + 5 * bs + 7, 65536 + 5 * bs, out)   # wrapped: up to the dictionary
    assert list(out) == [2 * bs + 7, 2 * bs]
    m.fp_decode_ring_too_small(bs, bs + 500, WINDOW - 500, 500, 0, bs + 9, bs, out)
    assert list(out) == [500 + bs + 9, bs + 500]


def decode_runs(kinds, bs=65536):
    kind = (C.c_uint8 * len(kinds))(*kinds)
    out = np.zeros((4 * len(kinds) + 4, 3), dtype=np.uint64)
    n = shim().fp_decode_runs(bs, kind, len(kinds), out.ctypes.data_as(C.POINTER(C.c_uint64)), len(out))
    assert n < len(out)
    return [tuple(int(v) for v in row) for row in out[:n]]


def test_decode_runs_tables():
    """launches (first block, blocks, room of the first block) of a run of 16 blocks, written out by hand from the rule: start with run =
    16; a launch takes min(run, what is left), the roomy block comes back alone; behind a launch that stopped early run = max(1, m / 4),
    behind a clean one min(16, 2 m); the launch that sends a block back for the ring's room leaves run alone, and the one block that
    comes back counts as a clean launch of one"""
    B = 65536
    assert decode_runs([0] * 16) == [(0, 16, B)]
    # every block short: 16 -> 4 -> 1, then a clean launch of one (2) and a launch of two that stops behind its first block (1) in turn
    assert decode_runs([1] * 16) == [(0, 16, B), (1, 4, B), (2, 1, B), (3, 2, B), (4, 1, B), (5, 2, B), (6, 1, B), (7, 2, B), (8, 1, B),
                                     (9, 2, B), (10, 1, B), (11, 2, B), (12, 1, B), (13, 2, B), (14, 1, B), (15, 1, B)]
    # block 5 short only: the launch accepts 0 .. 5 and stops early (4); clean launches double: 4, then 8 cut to the 6 that are left
    assert decode_runs([0] * 5 + [1] + [0] * 10) == [(0, 16, B), (6, 4, B), (10, 6, B)]
    # block 3 asks for the ring's room in a clean run: 0 .. 2 accepted, 3 alone with twice the room, then 2, 4, 8 cut to 6
    assert decode_runs([0] * 3 + [2] + [0] * 12) == [(0, 16, B), (3, 1, 2 * B), (4, 2, B), (6, 4, B), (10, 6, B)]
    # ... and with a short block 0 in front of it: (0, 16) stops behind block 0 (4); block 3 is the last of the next launch
    assert decode_runs([1, 0, 0, 2] + [0] * 12) == [(0, 16, B), (1, 4, B), (3, 1, 2 * B), (4, 2, B), (6, 4, B), (10, 6, B)]
    # launches and decoded blocks stay linear in the number of blocks, whatever the blocks
    rng = random.Random(26)
    for _ in range(50):
        kinds = [rng.choice([0, 0, 0, 1, 2]) for _ in range(rng.randrange(1, 300))]
        runs = decode_runs(kinds)
        assert sum(m for _, m, _ in runs) <= 4 * len(kinds) + 16
        assert runs[-1][0] + runs[-1][1] == len(kinds)


def test_launch_sizes():
    m = shim()
    # blocks per launch: an explicit batch size exactly (at least one block); automatic: at least 256 blocks, within 1 GiB
    assert [m.fp_blocks_per_launch(64 << 20, bs, 0) for bs in sorted(SIZES.values())] == [1024, 256, 64, 16]
    assert [m.fp_blocks_per_launch(64 << 20, bs, 1) for bs in sorted(SIZES.values())] == [1024, 256, 256, 256]
    assert m.fp_blocks_per_launch(1000, 65536, 0) == 1 and m.fp_blocks_per_launch(3 * 65536 + 5, 65536, 0) == 3
    assert m.fp_blocks_per_launch(1 << 40, 4 << 20, 1) == 1 << 18
    # the sink of a compressed block: what `len` bytes can decode to, at most a block
    assert [m.fp_decode_slot_cap(65536, n) for n in (0, 1, 256, 257, 65536)] == [64, 319, 65344, 65536, 65536]
    assert m.fp_decode_slot_cap(4 << 20, 16448) == 4194304 and m.fp_decode_slot_cap(4 << 20, 16447) == 255 * 16447 + 64
    # output reserved per launch: the batch size (at least a block), four times that when the batch size is automatic
    assert m.fp_launch_out_budget(64 << 20, 65536, 1) == 256 << 20 and m.fp_launch_out_budget(64 << 20, 65536, 0) == 64 << 20
    assert m.fp_launch_out_budget(1000, 65536, 0) == 65536
    # 32-bit sink positions: behind `carry` bytes, 2 n + 1 block sizes must stay below 2^32
    for carry, bs in ((0, 65536), (65536, 65536), (65536, 4 << 20), (12345, 1 << 20)):
        n = m.fp_pos_blocks(carry, bs)
        assert carry + (2 * n + 1) * bs <= 0xFFFFFFFF < carry + (2 * (n + 1) + 2) * bs
    assert m.fp_pos_blocks(65536, 65536) == 32766
