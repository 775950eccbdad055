"""GPU (-m gpu): the throughput encoder's indexer wavefront resolves a window's sizes (lz4_compress_wave.hip, resolve_window) while
the workers load the next window: lane j holds segment j's SegMeta, one uniform loop carries {out_pos, pend} over the eleven segments,
the carry to the block's next window goes through LDS (block mode) or the carry ring (window mode, which the indexer now polls itself).

What can go wrong is the arithmetic over segments of every kind (with and without a match, empty, a run window's single one), the carry
across the windows of a block and across skipped items, the record of a workgroup's last window (read behind one extra barrier), and in
window mode the wait for the carry, its poison and the second launch.  Every case: the bytes, out_len and status of every block == the
scalar model (tests/sim/wave_encoder_model.c through wave_model / dict_cases, as in test_gpu_wave_encoder.py), the oracle decodes them,
and the 0xEE canary behind every out_cap (and the whole sink of a block that reports an error) is untouched."""
import numpy as np
import pytest

import dict_cases as D
import oracle_api as O
import wave_model as W

pytestmark = pytest.mark.gpu

CANARY = 0xEE
PAD = 32


@pytest.fixture(scope="module")
def blk():
    from lz4_flex_amd import _lib, block
    lib = _lib.load()
    assert lib.lz4flex_device_count() >= 1
    assert lib.lz4flex_set_tuning(None, b"compress_mode", 0) == 0     # throughput mode on the default context
    return block


def workgroups():
    from lz4_flex_amd import _lib
    g = _lib.load().lz4flex_get_tuning(None, b"compress_workgroups")
    assert g >= 8
    return g


def SUB(n_blocks):
    """the sub-windows the library's default gives the blocks (of <= 64 KiB) of a batch of n_blocks (test_gpu_wave_encoder.py)"""
    return W.auto_sub(n_blocks, workgroups())


def layout(blocks, caps):
    in_len = [len(b) for b in blocks]
    in_off = [int(x) for x in np.concatenate([[0], np.cumsum([m + 3 for m in in_len])[:-1]])]      # unaligned block starts
    src = np.zeros(in_off[-1] + in_len[-1] + 64, dtype=np.uint8)
    for o, b in zip(in_off, blocks):
        src[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    out_off = [int(x) for x in np.concatenate([[0], np.cumsum([c + PAD for c in caps])[:-1]])]
    out = np.full(out_off[-1] + caps[-1] + PAD, CANARY, dtype=np.uint8)
    return src, in_off, in_len, out, out_off


def check(blocks, caps, out, out_off, out_len, status, want, small=(), decodes=None):
    """every block == `want` (its model), status 0; blocks in `small`: OutputTooSmall, nothing written; the canary; decodes(i, bytes)"""
    from lz4_flex_amd import _lib as L
    bad = []
    for i, b in enumerate(blocks):
        o, c = out_off[i], caps[i]
        assert (out[o + c:o + c + PAD] == CANARY).all(), "block %d wrote behind its out_cap" % i
        if i in small:
            assert status[i] == L.E_OUTPUT_TOO_SMALL and out_len[i] == 0, (i, int(status[i]), int(out_len[i]))
            assert (out[o:o + c] == CANARY).all(), "block %d (too small) wrote bytes" % i
            continue
        got = bytes(out[o:o + int(out_len[i])])
        if status[i] != 0 or got != want[i]:
            bad.append((i, len(b), int(status[i]), int(out_len[i]), len(want[i])))
            continue
        if decodes is None:
            assert O.decompress(got, len(b)) == ("ok", b), i
        else:
            assert decodes(i, got), i
    assert not bad, bad[:8]


_src = {}


def cut(kind, phase, n):
    """n bytes of JSON or text, cyclic, from `phase`"""
    if kind not in _src:
        _src[kind] = O.fixture_plain("compression_66k_JSON" if kind == "json" else "compression_65k")
    p = _src[kind]
    return (p * (n // len(p) + 3))[phase % len(p):phase % len(p) + n]


def block_mode_batch(G):
    """2 G + 8 blocks, so that workgroups 0 .. 7 encode three blocks one after the other (g, g + G, g + 2 G: a skipped item can be in the
    MIDDLE of a sequence) and every other workgroup two: blocks of 64 ... 3 000 bytes (one window shorter than a segment: ten empty
    segments), and among them the special ones.  Returns (blocks, the indices with a capacity too small)."""
    n = 2 * G + 8
    rnd = np.random.default_rng(23)
    blocks = [cut("json" if i % 3 else "text", 7919 * i, 64 + (i * 977) % 2937) for i in range(n)]
    # eight blocks of 130 KiB + 1 ... 200 KiB: three or four windows, the carry {out_pos, pend} goes through LDS from window to window
    big_at = [1, 3, 7, 40, G + 3, 2 * G + 2, 2 * G + 5, G + 300 if G > 300 else G + 4]
    big_len = [133121, 143000, 153001, 163840, 174003, 184321, 196608, 204800]
    for k, (i, m) in enumerate(zip(big_at, big_len)):
        blocks[i] = cut("text" if k % 2 else "json", 1000 * (k + 1), m)
    # incompressible, three windows: no segment has a match, pend accumulates over segments and windows, the last literals are the block
    blocks[G + 6] = rnd.integers(0, 256, 150001, dtype=np.uint8).tobytes()
    # run windows (>= 8 KiB of one byte): one alone, one in front of an ordinary (anchored) last window
    blocks[6] = bytes(12000)
    blocks[2 * G + 6] = bytes(65536) + cut("text", 555, 4000)
    # a last window whose parsed part (100 bytes) is shorter than one segment: empty segments behind a full window
    blocks[G + 7] = cut("json", 4242, 65536 + 100)
    # capacity one byte too small: skipped, between a three-window block and another one (workgroup 1), and between two small ones
    small = [G + 1, G + 5]
    return blocks, small


def test_block_mode_every_kind_of_segment(blk):
    G = workgroups()
    blocks, small = block_mode_batch(G)
    n = len(blocks)
    assert n >= G
    caps = [O.max_out(len(b)) - (1 if i in small else 0) for i, b in enumerate(blocks)]
    sub = SUB(n)
    want = [None if i in small else W.compress(b, sub=sub) for i, b in enumerate(blocks)]
    assert len(want[6]) < 100 and len(want[G + 6]) > 150001                 # (a run window's one sequence; literals only)
    src, in_off, in_len, out, out_off = layout(blocks, caps)
    for rep in range(2):                                                    # twice: the second launch starts from the records the first left
        out[:] = CANARY
        ol, st = blk.compress_batch(src, in_off, in_len, out, out_off, caps)
        check(blocks, caps, out, out_off, ol, st, want, small=set(small))


def window_mode_blocks():
    return [cut("json", 100, 200 * 1024), cut("text", 9000, 1 << 20), cut("json", 31, 65536 + 1)]


@pytest.mark.parametrize("carry_wait", [1, 0])
def test_window_mode_carry_through_the_indexer(blk, carry_wait):
    """three blocks, their windows dealt to the workgroups: the indexer polls the carry ring, resolves and hands the carry on.
    carry_wait 0: every window that has to wait gives up at once, leaves status 66 and tells its successors; the second launch
    encodes those blocks again -- the same bytes, status 0"""
    from lz4_flex_amd import _lib as L
    lib = L.load()
    blocks = window_mode_blocks()
    assert len(blocks) < workgroups()
    caps = [O.max_out(len(b)) for b in blocks]
    want = [W.compress(b, sub=SUB(len(blocks))) for b in blocks]
    src, in_off, in_len, out, out_off = layout(blocks, caps)
    assert lib.lz4flex_set_tuning(None, b"compress_carry_wait", carry_wait) == 0
    try:
        ol, st = blk.compress_batch(src, in_off, in_len, out, out_off, caps)
    finally:
        assert lib.lz4flex_set_tuning(None, b"compress_carry_wait", 1) == 0
    check(blocks, caps, out, out_off, ol, st, want)


def dict_batch(G):
    """G + 5 blocks of 64 ... 3 000 bytes from a pool of 24, and one of 100 000 bytes (windows that slide over the dictionary's tail)"""
    pool = [D.block("json" if k % 2 else "text", 64 + (k * 977) % 2937, salt=k) for k in range(24)]
    blocks = [pool[i % 24] for i in range(G + 5)]
    blocks[2] = D.block("json", 100000, salt=3)
    return blocks


_dmodel = {}


def dmodel(b, d):
    key = (b, d)
    if key not in _dmodel:
        _dmodel[key] = D.model(b, d) if d else W.compress(b, sub=1)
    return _dmodel[key]


def dicts3():
    d = D.dictionary("json")
    return [d[:100], d[:4096], d[:40000]]


def run_dict_form(blk, form):
    G = workgroups()
    blocks = dict_batch(G)
    n = len(blocks)
    caps = [O.max_out(len(b)) for b in blocks]
    src, in_off, in_len, out, out_off = layout(blocks, caps)
    ds = dicts3()
    if form == "per_block":
        which = [i % 3 for i in range(n)]
        dbuf = np.frombuffer(b"".join(ds), dtype=np.uint8)
        starts = [0, len(ds[0]), len(ds[0]) + len(ds[1])]
        ol, st = blk.compress_batch_with_dict(src, in_off, in_len, dbuf, [starts[k] for k in which], [len(ds[k]) for k in which], out, out_off, caps)
        used = [ds[k] for k in which]
    elif form == "shared":
        ol, st = blk.compress_batch_with_shared_dict(src, in_off, in_len, ds[2], out, out_off, caps)
        used = [ds[2]] * n
    else:
        ids = [blk.NO_DICT if i % 4 == 3 else i % 4 for i in range(n)]
        with blk.DictSet(ds) as dset:
            ol, st = blk.compress_batch_with_dict_set(src, in_off, in_len, ids, dset, out, out_off, caps)
        used = [b"" if k == blk.NO_DICT else ds[k] for k in ids]
    want = [dmodel(b, d) for b, d in zip(blocks, used)]
    check(blocks, caps, out, out_off, ol, st, want,
          decodes=lambda i, got: D.oracle_decodes(got, blocks[i], used[i]) if used[i] else O.decompress(got, len(blocks[i])) == ("ok", blocks[i]))


@pytest.mark.parametrize("form", ["per_block", "shared", "set"])
def test_dictionary_forms_share_the_body(blk, form):
    """lz4flex_compress_batch_ex, _shared_dict and _dict_set: their kernels are instances of the same wave_body"""
    run_dict_form(blk, form)
