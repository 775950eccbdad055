"""GPU (-m gpu): the split decoder's copiers write back and slide for the WHOLE wavefront in one visit (lz4_decompress_split.hip,
Copier::service() -> wave_flush() -> wave_flush_slide()): whenever one block of a copier wavefront runs out of buffer space, every
live block of that wavefront that has a complete 16-byte unit is written back and its history slid, with wave-uniform trip counts
and four LDS reads in flight.  So a block is flushed at moments its own fill never chose: with nothing, a few bytes, exactly one
unit or a nearly full buffer pending, in front of a near/far match boundary, next to blocks that have finished or failed.

Checker: the oracle (lz4_flex's decoder restated, tests/oracle_api).  Every case goes through lz4flex_decompress_batch with
"decompress_variant" 4 (the split decoder) at each "decompress_blocks_per_wg" the library offers: 64 (copier groups of 4 lanes x
16 bytes, 16 blocks per copier wavefront) and 8 / 16 / 32 (8 lanes x 4 bytes, 8 blocks per wavefront) -- Copier is one template.
Checked per block: bytes, length, status, OutputTooSmall{expected, actual}, and a 64-byte canary behind its capacity.

Batches hold 64 blocks written sequence by sequence (lz4_writer.Writer), most of <= 4 KiB of output: a few visits per group.
The buffer's numbers (lz4_split_parser.h, LayoutBig): 1 984 bytes, 512 of history, 1 440 usable (1 952 at a block's start); a
group asks for a visit with less than 320 bytes of space; a piece is 64 (32) bytes.  Which fill a block has when a NEIGHBOUR asks
for a visit is a matter of timing, not of the test's choice: every batch therefore puts fast blocks (900-byte literal runs: a
64-byte piece in every copier step) beside slow ones (sequences of 5 ... 70 bytes, one or two per parser step) in every copier
wavefront, and the slow blocks repeat their shapes at many phases."""
import ctypes as C

import numpy as np
import pytest

import oracle_api as O
from lz4_writer import Writer

pytestmark = pytest.mark.gpu
GEOMETRIES = [64, 8, 16, 32]
EDGES = [511, 512, 513, 1119, 1120, 1121, 1439, 1440, 1441, 1951, 1952, 1953, 2879, 2880, 2881]      # ... 2 x 1 440
NEAR_FAR = [(off, ml) for off in list(range(496, 529)) + [1, 2, 3] + list(range(4, 18)) for ml in (4, 16, 17, 64, 65)]
_POOL = np.random.RandomState(27).randint(0, 256, 1 << 16, dtype=np.uint8).tobytes()


def _rb(n, at):
    """n bytes of noise (a literal run that holds no match)"""
    at %= len(_POOL) - n
    return _POOL[at:at + n]


# ---------------------------------------------------------------------------------------------------------------- block shapes
def fast_block(total, k=0):
    """900-byte literal runs (below the long-run threshold of 1 024) with a short match between them: the group that asks for visits"""
    w = Writer()
    while len(w.out) + 900 + 8 + 5 <= total:
        w.seq(_rb(900, 131 * k + len(w.out)), 700 + 7 * (k % 9), 4 + k % 5)
    return w.end(max(total - len(w.out), 0) if total else 5)


def rle_block(total, k=0):
    """offset-1 (and 2, 3) matches: the periodic path, which flushes for itself"""
    w = Writer()
    i = 0
    while len(w.out) + 400 < total:
        w.seq(_rb(3 + (i + k) % 5, k + i), 1 + (i + k) % 3, 40 + 83 * ((i + k) % 4))
        i += 1
    return w.end(5)


def slow_block(total, step, k=0):
    """sequences of `step` + 0 ... 3 output bytes each, near matches: a few bytes of progress per parser step"""
    w = Writer().seq(_rb(32, k), 16, 8)
    i = 0
    while len(w.out) + step + 16 < total:
        lit = 1 + (i + k) % 3
        w.seq(_rb(lit, 5 * k + i), 8 + (i * 5 + k) % 24, step + (i % 4) - lit if step + (i % 4) - lit >= 4 else 4)
        i += 1
    return w.end(max(total - len(w.out), 0))


def tiny_block(n):
    """the whole output is n literal bytes"""
    return Writer().end(n)


def slice_block(stem, at, n):
    d = O.fixture_plain(stem)[at:at + n]
    return O.compress(d), d


def edge_block(size, then, k=0):
    """moderate sequences; with `then` > 0 a sequence ends at exactly `size` output bytes and `then` more bytes of sequences follow,
    the first of them a match that reads far back; with `then` == 0 the block's output ends at `size` (its last 5 ... 12 bytes are
    the last literals, which the format wants behind the last match)"""
    w = Writer().seq(_rb(48, k), 20, 30)
    i = 0
    tail = 0 if then else 5 + k % 8
    while size - tail - len(w.out) >= 140:
        w.seq(_rb(10 + (i + k) % 40, k + 3 * i), 9 + (7 * i + k) % 60, 20 + (i * 11 + k) % 50)
        i += 1
    rest = size - tail - len(w.out)                     # 22 ... 139: one sequence that ends at the boundary
    assert rest >= 8
    w.seq(_rb(rest - 6, k + 1), 33, 6)
    if not then:
        return w.end(tail)
    assert len(w.out) == size
    w.seq(_rb(3, k), 500 if size >= 500 else 64, 70)   # the first sequence behind the boundary reads far back
    while len(w.out) < size + then:
        w.seq(_rb(20, k + len(w.out)), 100, 44)
    return w.end(5)


def near_far_block(total, k):
    """600 bytes of literals, then literal 8 ... 40 + match (offset, length) over all of NEAR_FAR, starting at the k-th pair: matches
    whose source straddles the history's lower end L0 (offsets 496 ... 528: after a visit op - L0 is 512 ... 527), periodic ones (1 ... 3)
    and ones shorter than a 16-byte word (4 ... 17: cut at the offset)"""
    w = Writer().seq(_rb(600, 97 * k), 300, 12)
    i = 37 * k
    while len(w.out) + 120 < total:
        off, ml = NEAR_FAR[i % len(NEAR_FAR)]
        w.seq(_rb(8 + (i * 13 + k) % 33, i + k), off, ml)
        i += 1
    return w.end(5)


def long_run_block(run, k=0):
    """sequences up to mid-buffer, ONE literal run of `run` >= 1 024 bytes (memory to memory, the buffer rebuilt from its tail), then
    matches into the run's tail, 600 bytes back and near, and ordinary sequences"""
    w = Writer().seq(_rb(100, k), 50, 40)
    for i in range(4 + k % 5):
        w.seq(_rb(30 + i, k + i), 60 + i, 33)
    w.seq(_rb(run, 7 * k), 5, 9)
    w.seq(_rb(2, k), 600, 80).seq(_rb(1, k), 17, 65).seq(b"", 512, 64).seq(_rb(4, k), 1, 50)
    for i in range(12):
        w.seq(_rb(25, k + i), 40 + 37 * i, 30 + i)
    return w.end(7)


# ---------------------------------------------------------------------------------------------------------------- batches of 64
def _mix(slow, n_fast=16, fast_total=4096):
    """64 blocks: a fast block at every fourth place (two in every wavefront of 8 blocks, four in every one of 16), the slow ones between"""
    assert len(slow) == 64 - n_fast, len(slow)
    out, it = [], iter(slow)
    for i in range(64):
        if i % 4 == 1:
            out.append(fast_block(fast_total + 448 * (i % 3), i))
        else:
            out.append(next(it))
    return out


def batch_paces():
    """one wavefront, sixteen paces: fast, periodic, JSON / text slices, slow blocks of every step size, whole outputs of 0 ... 17 bytes"""
    slow = []
    for i in range(48):
        kind = i % 12
        if kind in (0, 6):
            slow.append(rle_block(3000, i))
        elif kind == 1:
            slow.append(slice_block("compression_66k_JSON", 1000 * i, 4096))
        elif kind == 7:
            slow.append(slice_block("compression_65k", 1200 * i, 3500))
        elif kind in (2, 8):
            slow.append(tiny_block((0, 1, 15, 16, 17, 31, 32, 33)[(i // 6) % 8]))
        else:
            slow.append(slow_block(1400 + 90 * i, 5 + (7 * i) % 66, i))
    return _mix(slow, fast_total=8192)


def batch_edges():
    """outputs that end, and sequence boundaries that fall, on the buffer's sizes and their neighbours"""
    slow = [edge_block(s, 0, i) for i, s in enumerate(EDGES)] + [edge_block(s, 700, i) for i, s in enumerate(EDGES)]
    slow += [fast_block(s, i) for i, s in enumerate(EDGES)]                       # ... and in 900-byte literal runs
    slow += [edge_block(1440 + 1120 * j + d, 0, j) for j in (1, 2) for d in (-1, 0)][:3]
    return _mix(slow)


def batch_near_far():
    return _mix([near_far_block(4096, k) for k in range(48)])


def batch_sinks():
    """capacity == size everywhere (as in every batch here); every third slow block one byte short (OutputTooSmall); truncated blocks
    and offset-0 blocks among good ones: a group that failed writes nothing more, its neighbours go on"""
    slow, caps = [], {}
    for i in range(48):
        c, d = near_far_block(3000, i) if i % 2 else slow_block(2600, 9 + i, i)
        if i % 3 == 0:
            caps[len(slow)] = len(d) - 1
        elif i % 8 == 1:
            c = c[:len(c) // 2 + i]                                    # cut in the middle
        elif i % 8 == 5:
            c = c[:-3]                                                 # cut in the last literals
        elif i % 8 == 7:
            w = Writer().seq(_rb(600, i), 300, 12)
            for j in range(20):
                w.seq(_rb(30, i + j), 70, 40)
            w.bad_seq(_rb(9, i), 0, 20)                                # offset 0 behind 2 000 good bytes
            for j in range(10):
                w.bad_seq(_rb(30, i + j), 70, 40)
            c = w.end(5)[0]
            d = bytes(3000)
        slow.append((c, d))
    blocks = _mix(slow)
    cap_list, it = [], 0
    for i, (c, d) in enumerate(blocks):
        if i % 4 == 1:
            cap_list.append(len(d) - (1 if i % 8 == 5 else 0))        # a fast block with a short sink, too
        else:
            cap_list.append(caps.get(it, len(d)))
            it += 1
    return blocks, cap_list


def batch_long_run():
    """one long literal run per wavefront of 8 (two per wavefront of 16), the neighbours in mid-buffer: bulk_literals' ordering"""
    slow = []
    for i in range(48):
        if i % 6 == 2:
            slow.append(long_run_block((1024, 1025, 1500, 3000, 5000, 1087, 1279, 2048)[(i // 6) % 8], i))
        elif i % 6 == 5:
            slow.append(slice_block("compression_66k_JSON", 900 * i, 3000))
        else:
            slow.append(slow_block(2500, 6 + (5 * i) % 60, i))
    return _mix(slow)


def _build():
    out = {}
    for name, fn in (("paces", batch_paces), ("edges", batch_edges), ("near_far", batch_near_far), ("long_run", batch_long_run)):
        blocks = fn()
        out[name] = ([c for c, _ in blocks], [len(d) for _, d in blocks])
    blocks, caps = batch_sinks()
    out["sinks"] = ([c for c, _ in blocks], caps)
    return out


@pytest.fixture(scope="module")
def batches():
    """name -> (blocks, capacities, the oracle's result per block): built and decoded by the oracle once for all geometries"""
    out = {}
    for name, (comps, caps) in _build().items():
        assert len(comps) == 64
        out[name] = (comps, caps, [O.decompress(c, k) for c, k in zip(comps, caps)])
    return out


@pytest.fixture(scope="module")
def env():
    from lz4_flex_amd import _lib, block
    lib = _lib.load()
    assert lib.lz4flex_device_count() >= 1
    return lib, block


def _decode(lib, block, bpw, comps, caps):
    inb = np.frombuffer(b"".join(comps) + bytes(64), dtype=np.uint8)
    in_len = [len(c) for c in comps]
    in_off = np.concatenate([[0], np.cumsum(in_len[:-1], dtype=np.uint64)]).astype(np.uint64)
    out_off = np.concatenate([[0], np.cumsum([k + 64 for k in caps[:-1]], dtype=np.uint64)]).astype(np.uint64)
    out = np.full(int(out_off[-1]) + caps[-1] + 64, 0xA5, dtype=np.uint8)
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), -1) == 0
    try:
        assert lib.lz4flex_set_tuning(ctx, b"decompress_variant", 4) == 0
        assert lib.lz4flex_set_tuning(ctx, b"decompress_blocks_per_wg", bpw) == 0
        ol, st, det = block.decompress_batch(inb, in_off, in_len, out, out_off, caps, ctx=ctx)
    finally:
        lib.lz4flex_ctx_destroy(ctx)
    return out, out_off, ol, st, det


def _check(name, bpw, comps, caps, want, res):
    out, out_off, ol, st, det = res
    for i, (k, w) in enumerate(zip(caps, want)):
        o = int(out_off[i])
        tag = "%s, %d blocks per workgroup, block %d (%d -> capacity %d)" % (name, bpw, i, len(comps[i]), k)
        if w[0] == "ok":
            assert st[i] == 0 and ol[i] == len(w[1]), (tag, int(st[i]), int(ol[i]), len(w[1]))
            got = out[o:o + len(w[1])].tobytes()
            if got != w[1]:
                first = next(j for j in range(len(got)) if got[j] != w[1][j])
                raise AssertionError("%s: bytes differ from the oracle's at %d of %d" % (tag, first, len(got)))
            assert out[o + len(w[1]):o + k].tobytes() == b"\xA5" * (k - len(w[1])), tag + ": wrote behind its end"
        else:
            assert O.ERR_NAMES.get(int(st[i])) == w[0], (tag, int(st[i]), w[0])
            if w[0] == "OutputTooSmall":
                assert (int(det[i][0]), int(det[i][1])) == tuple(w[1]), (tag, det[i], w[1])
        assert out[o + k:o + k + 64].tobytes() == b"\xA5" * 64, tag + ": wrote behind its sink"


def test_the_batches_are_what_they_claim(batches):
    """(no kernel) the shapes the docstrings promise are in the batches: sizes on the buffer's edges, every near/far pair, every error
    class of the sinks batch, long runs on both sides of 1 024 + a piece"""
    comps, caps, want = batches["edges"]
    sizes = {len(w[1]) for w in want if w[0] == "ok"}
    assert set(EDGES) <= sizes and all(w[0] == "ok" for w in want)
    comps, caps, want = batches["sinks"]
    kinds = {w[0] for w in want}
    assert {"ok", "OutputTooSmall", "OffsetZero"} <= kinds and len(kinds) >= 4, kinds        # (+ what a cut block gives)
    assert sum(w[0] == "ok" for w in want) >= 24
    for name in ("paces", "near_far", "long_run"):
        assert all(w[0] == "ok" for w in batches[name][2]), name
    assert {len(w[1]) for w in batches["paces"][2]} >= {0, 1, 15, 16, 17}
    assert max(max(b[1]) for b in batches.values()) <= 9200 and sorted(batches["near_far"][1])[40] <= 4200


@pytest.mark.parametrize("bpw", GEOMETRIES)
@pytest.mark.parametrize("name", ["paces", "edges", "near_far", "sinks", "long_run"])
def test_wavefront_visit_equals_oracle(env, batches, name, bpw):
    lib, block = env
    comps, caps, want = batches[name]
    _check(name, bpw, comps, caps, want, _decode(lib, block, bpw, comps, caps))
