"""GPU (-m gpu): the sequence decoder (lz4_flex_amd/csrc/lz4_decompress_seq.hip, decompress_variant 13: one block per wavefront, one lane
per sequence) on ITS OWN boundaries -- the generic decoder matrix of test_gpu_block.py (KATs, adversarial batch, every prefix / corruption,
synthetic dependency blocks), test_gpu_pcd.py (large blocks) and test_gpu_dispatch_matrix.py (the thresholds +- 1) runs it as DECODERS -13;
here are blocks WRITTEN sequence by sequence to sit on the kernel's geometry:
  a lane copies literal runs <= 64 bytes, matches <= 273 bytes that do not overlap their source, far matches <= 64 bytes; anything else is
  executed alone by the wavefront, runs of >= 1 KiB memory to memory (periodic form for offsets < 1 KiB); tiles of 3 840 compressed bytes
  in 64 parts of 60; chunks of <= 64 sequences and <= 1 120 output bytes; a 3 584-byte window that slides by keeping 1 280 bytes.
Checker: the oracle (lz4_flex's decoder restated), which also says what an invalid variant of each block is (status, OutputTooSmall detail).
With the second pass off, the kernel must have decoded every valid block ITSELF (a silent fall-back to the reference-order kernel would pass
every other test)."""
import ctypes as C
import random

import numpy as np
import pytest

import oracle_api as O
from seq_blocks import blocks as _blocks

pytestmark = pytest.mark.gpu
REDO = 0x7F000001


@pytest.fixture(scope="module")
def env():
    from lz4_flex_amd import _lib, block
    lib = _lib.load()
    assert lib.lz4flex_device_count() >= 1
    return lib, block


def _ctx(lib, second_pass=1):
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), -1) == 0
    assert lib.lz4flex_set_tuning(ctx, b"decompress_variant", 13) == 0
    assert lib.lz4flex_set_tuning(ctx, b"decompress_second_pass", second_pass) == 0
    return ctx


def _batch(block, ctx, comps, caps, slack=64, misalign=0):
    inb = np.frombuffer(bytes(misalign) + b"".join(comps) + bytes(64), dtype=np.uint8)
    in_len = [len(c) for c in comps]
    in_off = (np.concatenate([[0], np.cumsum(in_len[:-1], dtype=np.uint64)]) + misalign).astype(np.uint64)
    out_off = (np.concatenate([[0], np.cumsum([k + slack for k in caps[:-1]], dtype=np.uint64)]) + misalign).astype(np.uint64)
    out = np.full(int(out_off[-1]) + caps[-1] + slack, 0xA5, dtype=np.uint8)
    ol, st, det = block.decompress_batch(inb, in_off, in_len, out, out_off, caps, ctx=ctx)
    return out, out_off, ol, st, det


def test_blocks_on_the_decoders_own_boundaries(env):
    """every block above: bytes == oracle with an exact sink, with a sink 777 bytes larger, nothing behind either; a sink 1 / 40 bytes short and a
    block cut short end like the oracle says (status, OutputTooSmall detail) -- through the second pass, which is the reference-order kernel"""
    lib, block = env
    blocks = _blocks()
    comps, caps, want = [], [], []
    for name, c, p in blocks:
        for cap in (len(p), len(p) + 777):
            comps.append(c); caps.append(cap); want.append((name, ("ok", p)))
        for cap in (max(len(p) - 1, 0), max(len(p) - 40, 0)):
            comps.append(c); caps.append(cap); want.append((name + " (short sink)", O.decompress(c, cap)))
        comps.append(c[:-3]); caps.append(len(p)); want.append((name + " (cut)", O.decompress(c[:-3], len(p))))
    for misalign in (0, 5):                         # the batch's buffers at an odd address: every block's input and output are unaligned
        ctx = _ctx(lib)
        try:
            out, out_off, ol, st, det = _batch(block, ctx, comps, caps, misalign=misalign)
        finally:
            lib.lz4flex_ctx_destroy(ctx)
        for i, (name, w) in enumerate(want):
            o = int(out_off[i])
            if w[0] == "ok":
                assert st[i] == 0 and ol[i] == len(w[1]), (name, i, int(st[i]), int(ol[i]), len(w[1]))
                assert out[o:o + len(w[1])].tobytes() == w[1], "%s: bytes differ" % name
                assert out[o + len(w[1]):o + caps[i] + 64].tobytes() == b"\xA5" * (caps[i] - len(w[1]) + 64), "%s: wrote behind its end" % name
            else:
                assert O.ERR_NAMES.get(int(st[i])) == w[0], (name, int(st[i]), w[0])
                if w[0] == "OutputTooSmall":
                    assert (int(det[i][0]), int(det[i][1])) == tuple(w[1]), (name, det[i], w[1])
                assert out[o + caps[i]:o + caps[i] + 64].tobytes() == b"\xA5" * 64, "%s: wrote behind its sink" % name


def test_the_kernel_decodes_every_valid_block_itself(env):
    """second pass off: a valid block must come out of THIS kernel (status 0, the oracle's bytes), an invalid one must be left marked
    (0x7F000001) -- nothing is quietly handed to the reference-order kernel"""
    lib, block = env
    blocks = _blocks()
    comps = [c for _, c, _ in blocks] + [c[:-2] for _, c, p in blocks if len(c) > 8]
    caps = [len(p) for _, _, p in blocks] + [len(p) for _, c, p in blocks if len(c) > 8]
    plains = [p for _, _, p in blocks]
    ctx = _ctx(lib, second_pass=0)
    try:
        out, out_off, ol, st, det = _batch(block, ctx, comps, caps)
    finally:
        lib.lz4flex_ctx_destroy(ctx)
    for i, p in enumerate(plains):
        o = int(out_off[i])
        assert st[i] == 0 and ol[i] == len(p) and out[o:o + len(p)].tobytes() == p, (blocks[i][0], int(st[i]), int(ol[i]), len(p))
    for i in range(len(plains), len(comps)):
        verdict = O.decompress(comps[i], caps[i])
        assert (st[i] == 0) == (verdict[0] == "ok"), (i, int(st[i]), verdict[0])
        assert st[i] in (0, REDO), (i, int(st[i]))


def test_a_medium_batch_through_the_default_dispatch(env):
    """1 500 blocks (the default dispatch's range for this decoder: 641 ... 14 336) of every kind above and of both encoders' JSON / text tiles, one
    launch, `decompress_variant` 0: == oracle"""
    import wave_model as W
    lib, block = env
    rnd = random.Random(9)
    j, t = O.fixture_plain("compression_66k_JSON"), O.fixture_plain("compression_65k")
    pool = [(c, p) for _, c, p in _blocks() if len(p) <= 200000]
    for k in range(40):
        src = (j if k % 2 else t) * 3
        ph = rnd.randrange(len(src) // 3)
        p = src[ph:ph + rnd.choice((65536, 65536, 30000, 1000))]
        pool.append(((O.compress if k % 3 else W.compress)(p), p))
    picks = [pool[rnd.randrange(len(pool))] for _ in range(1500)]
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), -1) == 0
    try:
        assert 641 <= len(picks) <= lib.lz4flex_get_tuning(ctx, b"dispatch_threshold_4")
        out, out_off, ol, st, det = _batch(block, ctx, [c for c, _ in picks], [len(p) for _, p in picks])
    finally:
        lib.lz4flex_ctx_destroy(ctx)
    for i, (c, p) in enumerate(picks):
        o = int(out_off[i])
        assert st[i] == 0 and ol[i] == len(p) and out[o:o + len(p)].tobytes() == p, i
