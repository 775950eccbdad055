"""GPU (-m gpu): the throughput ("wave") encoder, lz4_compress_wave.hip, on the shape corpus of tests/wave_shapes.py -- sequences on
both sides of every length-byte boundary of each place the kernel writes one (encode_seqs' lanes, emit_generic, place_segment, a run
window), under every configuration that moves segment and window starts (test_wave_trace.py asserts that the model's output holds
them all).  The kernel must write the scalar model's bytes for every block; the reference-exact encoder the oracle's."""
import ctypes as C

import numpy as np
import pytest

import oracle_api as O
import wave_model as W
import wave_shapes as S

pytestmark = pytest.mark.gpu

_CORPUS = {}


def corpus(config):
    if config not in _CORPUS:
        _CORPUS[config] = S.blocks(config)
    return _CORPUS[config]


@pytest.fixture(scope="module")
def blk():
    from lz4_flex_amd import _lib, block
    lib = _lib.load()
    assert lib.lz4flex_device_count() >= 1
    assert lib.lz4flex_set_tuning(None, b"compress_mode", 0) == 0     # throughput mode on the default context
    return block


@pytest.mark.parametrize("config", sorted(S.CONFIGS))
def test_wave_sequences_scalar_call(blk, config):
    """one block per call (blocks of <= 64 KiB: four sub-windows; longer ones: the default window stride); a history config's blocks
    without their history"""
    for k, (data, kw) in enumerate(corpus(config)):
        d = data[kw.get("hist", 0):]
        comp = blk.compress(d)
        assert comp == W.compress(d), (config, k, len(comp), len(W.compress(d)))
        assert O.decompress(comp, len(d)) == ("ok", d), (config, k)
        assert O.c_decompress(comp, len(d)) == d, (config, k)


def _device_batch(L, lib, ctx, blocks, hist, kw):
    """the blocks in one device-resident batch at odd input and output offsets, each behind its own history (hist bytes, promised by
    LZ4FLEX_BLOCK_HISTORY flags when hist != 0); every block == model; then the default GPU decoder returns every block"""
    import torch
    dev = torch.device("cuda", 0)
    parts = [b[hist:] for b in blocks]
    in_len = np.array([len(b) for b in parts], dtype=np.uint32)
    in_off = np.zeros(len(parts), dtype=np.uint64)
    buf = bytearray()
    for k, b in enumerate(blocks):
        buf += bytes(2 * k + 1)                                         # odd gaps: every block starts at an odd offset
        buf += b[:hist]
        in_off[k] = len(buf)
        buf += b[hist:]
    buf += bytes(64)
    cap = np.array([O.max_out(len(b)) for b in parts], dtype=np.uint32)
    out_off = np.zeros(len(parts), dtype=np.uint64)
    pos = 3
    for k in range(len(parts)):
        out_off[k] = pos
        pos += int(cap[k]) + 2 * k + 5                                  # odd output offsets
    flags = np.array([hist << 8] * len(parts), dtype=np.uint32)
    tt = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)
    d_in = torch.from_numpy(np.frombuffer(bytes(buf), dtype=np.uint8).copy()).to(dev)
    d_out = torch.zeros(pos + 64, dtype=torch.uint8, device=dev)
    d_in_off, d_in_len, d_flags = tt(in_off, np.int64), tt(in_len, np.int32), tt(flags, np.int32)
    d_out_off, d_cap = tt(out_off, np.int64), tt(cap, np.int32)
    d_len = torch.zeros(len(parts), dtype=torch.int32, device=dev)
    d_st = torch.full((len(parts),), -1, dtype=torch.int32, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr())
    rc = lib.lz4flex_compress_batch(ctx, p(d_in), p(d_in_off), p(d_in_len), p(d_flags) if hist else None, len(parts), p(d_out),
                                    p(d_out_off), p(d_cap), p(d_len), p(d_st), L.MEM_DEVICE, None)
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    assert d_st.cpu().tolist() == [0] * len(parts)
    h_out, h_len = d_out.cpu().numpy(), d_len.cpu().numpy()
    for k, b in enumerate(blocks):
        got = bytes(h_out[int(out_off[k]):int(out_off[k]) + int(h_len[k])])
        assert got == W.compress(b, **kw), (k, kw, len(got))
        assert O.decompress(got, len(parts[k]), dict_data=b[:hist] if hist else None) == ("ok", parts[k]), (k, kw)
    if hist:
        return                  # (these blocks need their history as a dictionary: the oracle decoded them above)
    d_back = torch.zeros_like(d_in)
    d_blen = torch.zeros(len(parts), dtype=torch.int32, device=dev)
    d_bst = torch.full((len(parts),), -1, dtype=torch.int32, device=dev)
    rc = lib.lz4flex_decompress_batch(ctx, p(d_out), p(d_out_off), p(d_len), len(parts), p(d_back), p(d_in_off), p(d_in_len),
                                      p(d_blen), p(d_bst), None, L.MEM_DEVICE, None)
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    assert d_bst.cpu().tolist() == [0] * len(parts) and torch.equal(d_blen, d_in_len)
    hb = d_back.cpu().numpy()
    for k in range(len(parts)):
        assert bytes(hb[int(in_off[k]):int(in_off[k]) + len(parts[k])]) == parts[k], k


@pytest.mark.parametrize("config,carry_wait", [(c, 1) for c in sorted(S.CONFIGS)] +
                         [(c, 0) for c in sorted(S.CONFIGS) if c not in S.SINGLE_WINDOW])
def test_wave_sequences_device_batch(blk, config, carry_wait):
    """one device batch per configuration (fewer blocks than workgroups: windows and sub-windows are dealt to different workgroups and
    carries -- empty windows' included -- travel through the workspace ring); carry_wait 0: a waiting window gives up at once, the
    second launch encodes its block again, to the same bytes"""
    from lz4_flex_amd import _lib as L
    lib = L.load()
    blocks = [d for d, _ in corpus(config)]
    kw = dict(corpus(config)[0][1])
    hist = kw.get("hist", 0)
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
    try:
        assert lib.lz4flex_set_tuning(ctx, b"compress_mode", 0) == 0
        assert lib.lz4flex_set_tuning(ctx, b"compress_carry_wait", carry_wait) == 0
        if "sub" in kw:
            assert lib.lz4flex_set_tuning(ctx, b"compress_subwindows", kw["sub"]) == 0
        if "slide" in kw:
            assert lib.lz4flex_set_tuning(ctx, b"compress_sliding_window", kw["slide"]) == 0
        _device_batch(L, lib, ctx, blocks, hist, kw)
    finally:
        lib.lz4flex_ctx_destroy(ctx)


def test_wave_sequences_sub_by_batch_size(blk):
    """compress_subwindows 0 (the default): the sub-windows the batch size gives (wave_model.auto_sub) -- the 64 KiB corpus blocks of
    every sub configuration, repeated to batches that get four, three, two and one sub-windows"""
    from lz4_flex_amd import _lib as L
    lib = L.load()
    wg = lib.lz4flex_get_tuning(None, b"compress_workgroups")
    blocks = [d for c in ("sub1", "sub2", "sub3", "sub4") for d, _ in corpus(c)]
    for n_blocks in (len(blocks), wg // 3, wg // 2 - 10, wg + 1):
        batch = (blocks * (n_blocks // len(blocks) + 1))[:n_blocks]
        sub = W.auto_sub(n_blocks, wg)
        src = np.frombuffer(b"".join(batch) + bytes(64), dtype=np.uint8).copy()
        in_len = [len(b) for b in batch]
        in_off = [int(x) for x in np.concatenate([[0], np.cumsum(in_len)[:-1]])]
        cap = [O.max_out(n) for n in in_len]
        out_off = [int(x) for x in np.concatenate([[0], np.cumsum(cap)[:-1]])]
        outb = np.zeros(sum(cap) + 64, dtype=np.uint8)
        ol, st = blk.compress_batch(src, in_off, in_len, outb, out_off, cap)
        assert not st.any()
        want = {}
        for k, b in enumerate(batch):
            got = bytes(outb[out_off[k]:out_off[k] + int(ol[k])])
            if b not in want:
                want[b] = W.compress(b, sub=sub)
            assert got == want[b], (n_blocks, sub, k)


def test_wave_sequences_exact_mode(blk):
    """compress_mode exact (lz4_compress.hip) on the same corpus: the oracle's bytes"""
    blk.set_compress_mode("exact")
    try:
        for config in sorted(S.CONFIGS):
            for k, (data, kw) in enumerate(corpus(config)):
                d = data[kw.get("hist", 0):]
                assert blk.compress(d) == O.compress(d), (config, k)
    finally:
        blk.set_compress_mode("fast")
