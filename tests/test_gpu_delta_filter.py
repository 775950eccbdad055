"""GPU tests of LZ4FLEX_FILTER_DELTA (the DELTA kernels of lz4_filter.hip behind lz4flex_filter_batch, lz4flex_compress_batch_typed,
lz4flex_decompress_batch_typed and the tensor forms of lz4_flex_amd.block): forward and inverse against the numpy model of
tests/delta_filter_model.py, byte for byte, with canaries around everything they write -- at the element counts where a restart meets a
lane, a tile, a bit-shuffle residue or a tail, at aligned and unaligned offsets, by the wide and the narrow path -- and the typed codec
calls against the plain ones over model-filtered bytes.  The harness (layouts, canaries, the plain calls) is test_gpu_filter's."""
import numpy as np
import pytest

import delta_filter_model as D
import filter_model as M
import oracle_api as O
import test_gpu_filter as T
from test_gpu_filter import ctx, lib      # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu

FLAGGED = [D.DELTA | M.NONE, D.DELTA | M.SHUFFLE, D.DELTA | M.BITSHUFFLE]
COUNTS = [0, 1, 2, 15, 16, 17, 1023, 1024, 1025, 1027, 1031, 2049, 3089, 65536]
RESIDUES = [(0, 0), (1, 5), (5, 0), (0, 1)]              # (input, output) offsets mod 16; the inverse's wide path needs the output's 0
E_OUTPUT_TOO_SMALL = 1


def patterns(E, n, rnd):
    """n elements of E bytes: random, all 0xFF, monotone, and values that carry and borrow across the dword (E = 8: 0x00000000FFFFFFFF /
    0x0000000100000000), across the packed halves (E = 2: 0x00FF / 0x0100), across the sign bit of a byte (E = 1: 0x7F / 0x80 / 0xFF)"""
    u = D.UINT[E]
    alt = {8: (0x00000000FFFFFFFF, 0x0000000100000000), 4: (0x0000FFFF, 0x00010000), 2: (0x00FF, 0x0100), 1: (0x7F, 0x80, 0xFF)}[E]
    return [rnd.integers(0, 256, n * E, dtype=np.uint8), np.full(n * E, 0xFF, np.uint8),
            (np.cumsum(rnd.integers(0, 200, n)).astype(np.uint64) + np.uint64(1_700_000_000_000)).astype(u).view(np.uint8),
            np.resize(np.array(alt, np.uint64), n).astype(u).view(np.uint8)]


@pytest.fixture(scope="module")
def delta_batches():
    """per E: blocks of every element count, each with 0 and E - 1 tail bytes -- at offsets (0, 0) with every data pattern, at the other
    residues with one pattern each (the long block: two patterns aligned, one elsewhere) -- and the lengths below E; per flagged filter the
    model's forward transform of each block.  All lengths go through one call."""
    rnd = np.random.default_rng(2121)
    res = {}
    for E in M.ELEMS:
        blocks, in_res, out_res = [], [], []
        for r, (ri, ro) in enumerate(RESIDUES):
            for k, m in enumerate(COUNTS):
                for tail in sorted({0, E - 1}):
                    pats = patterns(E, m, rnd)
                    pick = range(4) if r == 0 else [(k + r) % 4]
                    if m > 4096:
                        pick = ([0, 3] if tail == 0 else [2]) if r == 0 else ([(k + r) % 4] if tail == 0 else [])
                    for p in pick:
                        blocks.append(np.concatenate([pats[p], rnd.integers(0, 256, tail, dtype=np.uint8)]))
                        in_res.append(ri)
                        out_res.append(ro)
        for n in range(E):
            blocks.append(rnd.integers(0, 256, n, dtype=np.uint8))
            in_res.append(5)
            out_res.append(1)
        res[E] = (blocks, in_res, out_res, {f: [D.forward(b, f & 3, E) for b in blocks] for f in FLAGGED})
    return res


@pytest.mark.parametrize("inv", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("E", M.ELEMS)
@pytest.mark.parametrize("filt", FLAGGED, ids=["delta", "delta+shuffle", "delta+bitshuffle"])
def test_filter_batch_with_the_flag_is_the_model(lib, ctx, delta_batches, filt, E, inv):
    blocks, in_res, out_res, fwd = delta_batches[E]
    src, want = (fwd[filt], blocks) if inv else (blocks, fwd[filt])
    for b, f in zip(blocks[:8], fwd[filt][:8]):
        assert (D.inverse(f, filt & 3, E) == b).all()
    for bytewise in (0, 1):
        assert lib.lz4flex_set_tuning(ctx, b"filter_bytewise", bytewise) == 0
        T.check_filter(lib, ctx, "device", src, in_res, out_res, filt, E, inv, want,
                       "filter 0x%x E %d inverse %d bytewise %d" % (filt, E, inv, bytewise))
    # through host memory: every block below 4 096 elements, bytewise 0 and 1
    sel = [i for i, b in enumerate(blocks) if b.size <= 4096 * E]
    pick = lambda xs: [xs[i] for i in sel]
    for bytewise in (0, 1):
        assert lib.lz4flex_set_tuning(ctx, b"filter_bytewise", bytewise) == 0
        T.check_filter(lib, ctx, "host", pick(src), pick(in_res), pick(out_res), filt, E, inv, pick(want),
                       "host filter 0x%x E %d inverse %d bytewise %d" % (filt, E, inv, bytewise))


@pytest.mark.parametrize("filt", FLAGGED, ids=["delta", "delta+shuffle", "delta+bitshuffle"])
def test_more_blocks_than_wavefronts(lib, ctx, filt):
    """8 200 blocks of 40 bytes in one call: the grid has 8 192 wavefronts, so some take a second block"""
    rnd = np.random.default_rng(filt)
    rows = np.cumsum(rnd.integers(0, 9, (8200, 40), dtype=np.uint8), axis=1, dtype=np.uint8)
    blocks = [row for row in rows]
    in_res, out_res = [k % 16 for k in range(8200)], [(3 * k + 1) % 16 if k % 3 else 0 for k in range(8200)]
    for E in M.ELEMS:
        fwd = [D.forward(b, filt & 3, E) for b in blocks]
        T.check_filter(lib, ctx, "device", blocks, in_res, out_res, filt, E, False, fwd, "8 200 x 40 filter 0x%x E %d forward" % (filt, E))
        T.check_filter(lib, ctx, "device", fwd, in_res, out_res, filt, E, True, blocks, "8 200 x 40 filter 0x%x E %d inverse" % (filt, E))


# ---- the typed codec calls -------------------------------------------------------------------------------------------------------
TYPED = [("device", D.DELTA | M.BITSHUFFLE, 8), ("device", D.DELTA | M.SHUFFLE, 2), ("device", D.DELTA | M.NONE, 4),
         ("host", D.DELTA | M.BITSHUFFLE, 4), ("host", D.DELTA | M.NONE, 1)]


@pytest.mark.parametrize("mode", [0, 1], ids=["fast", "exact"])
@pytest.mark.parametrize("mem,filt,E", TYPED)
def test_typed_compress_with_the_flag_is_compress_batch_of_the_filtered_bytes(lib, ctx, mem, filt, E, mode):
    blocks = T.numeric_blocks(E, 37 * E + filt)
    filtered = [D.forward(b, filt & 3, E) for b in blocks]
    caps = [O.max_out(b.size) for b in blocks]
    short = 9                                            # 70 000 bytes with a slot below what they need
    assert blocks[short].size == 70000
    caps[short] = blocks[short].size // 2
    assert lib.lz4flex_set_tuning(ctx, b"compress_mode", mode) == 0
    want = T.run_compress(lib, ctx, mem, "plain", filtered, caps)
    got = T.run_compress(lib, ctx, mem, "typed", blocks, caps, filt, E)
    T.same_compress_results(got, want, "typed compress %s filter 0x%x E %d mode %d" % (mem, filt, E, mode))
    assert got["status"][short] == E_OUTPUT_TOO_SMALL and (np.delete(got["status"], short) == 0).all()
    image = np.full(got["out"].size, T.CANARY, np.uint8)
    for o, cap in zip(got["out_off"], caps):
        image[int(o):int(o) + cap] = got["out"][int(o):int(o) + cap]
    assert (got["out"] == image).all()
    for i in (0, 3, 7, 10, 14, len(blocks) - 1):         # a sample decodes, by the oracle and the model's inverse, to the input
        o, ln = int(got["out_off"][i]), int(got["out_len"][i])
        st, back = O.decompress(got["out"][o:o + ln].tobytes(), blocks[i].size)
        assert st == "ok" and (D.inverse(np.frombuffer(back, np.uint8), filt & 3, E) == blocks[i]).all(), (i, blocks[i].size, st)


@pytest.mark.parametrize("mem,filt,E", TYPED)
def test_typed_decompress_with_the_flag_gives_the_numbers_back(lib, ctx, mem, filt, E):
    blocks = T.numeric_blocks(E, 19 * E + filt)
    if mem == "host":
        blocks = blocks[:16]
    comps = [O.compress(D.forward(b, filt & 3, E).tobytes()) for b in blocks]
    caps = [b.size + (7 if k % 4 == 1 else 0) for k, b in enumerate(blocks)]
    damaged, short = 7, 9
    assert blocks[damaged].size == 65536 and blocks[short].size > 1000
    comps[damaged] = comps[damaged][:len(comps[damaged]) // 2] + bytes(3)
    caps[short] = blocks[short].size - 1
    want = T.run_decompress(lib, ctx, mem, "plain", comps, caps)
    got = T.run_decompress(lib, ctx, mem, "typed", comps, caps, filt, E)
    T.same_decode_results(got, want, mem)
    assert got["status"][damaged] != 0 and got["status"][short] == E_OUTPUT_TOO_SMALL and (np.delete(got["status"], [damaged, short]) == 0).all()
    # the good blocks are the model's inverse of the plain decode -- the inputs; the failed blocks' slots and all between are canary
    image = np.full(got["out"].size, T.CANARY, np.uint8)
    for i, (b, o) in enumerate(zip(blocks, got["out_off"])):
        if i not in (damaged, short):
            o = int(o)
            plain = want["out"][o:o + b.size]
            assert (D.inverse(plain, filt & 3, E) == b).all(), i
            image[o:o + b.size] = b
    wrong = np.nonzero(got["out"] != image)[0]
    assert wrong.size == 0, "typed decompress %s filter 0x%x E %d: %d bytes differ, first at %d" % (mem, filt, E, wrong.size, wrong[0])


def test_delta_makes_timestamps_smaller_in_exact_mode(lib, ctx):
    """compress_mode exact gives the oracle's bytes, so the figures are the CPU's: int64_timestamps(65536, 1) is 0.220 of its size behind
    BITSHUFFLE and 0.150 behind DELTA | BITSHUFFLE, 0.68 x; the bound is 0.8 x"""
    x = M.int64_timestamps(65536, 1)
    assert lib.lz4flex_set_tuning(ctx, b"compress_mode", 1) == 0
    size = {}
    for filt in (M.BITSHUFFLE, D.DELTA | M.BITSHUFFLE):
        got = T.run_compress(lib, ctx, "device", "typed", [x], [O.max_out(x.size)], filt, 8)
        assert got["status"][0] == 0
        o, ln = int(got["out_off"][0]), int(got["out_len"][0])
        assert got["out"][o:o + ln].tobytes() == O.compress(D.forward(x, filt & 3, 8, bool(filt & D.DELTA)).tobytes())
        size[filt] = ln
    print("timestamps, exact: bitshuffle %.3f, delta + bitshuffle %.3f of the input" % (size[2] / x.size, size[0x12] / x.size))
    assert size[0x12] < 0.8 * size[2], size


# ---- tensors -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", ["bitshuffle", "shuffle", "none"])
def test_tensor_round_trip_with_delta_is_bitwise(lib, filt):
    import torch
    from lz4_flex_amd import block
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(11)
    n = 50003                                            # the byte sizes are multiples of neither block_bytes
    stamps = torch.cumsum(torch.randint(900, 1100, (n,), generator=g), 0) + 1_700_000_000_000
    tensors = [stamps, torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g).to(torch.int32), (stamps % 65536 - 32768).to(torch.int16),
               torch.randint(0, 256, (n,), generator=g).to(torch.uint8), (torch.randn(n, generator=g) * 0.02).to(torch.bfloat16)]
    assert [t.dtype for t in tensors] == [torch.int64, torch.int32, torch.int16, torch.uint8, torch.bfloat16]
    for t in tensors:
        for block_bytes in (65536, 4096):
            assert (t.numel() * t.element_size()) % block_bytes != 0
            rec = block.compress_tensor(t.to(dev), block_bytes=block_bytes, filter=filt, delta=True)
            assert rec.delta is True and rec.filter == block.FILTERS[filt] and rec.dtype == t.dtype and rec.block_bytes == block_bytes
            back = block.decompress_tensor(rec)
            assert back.dtype == t.dtype and back.shape == t.shape and back.device.type == "cuda"
            assert torch.equal(back.cpu().view(torch.uint8), t.view(torch.uint8)), (t.dtype, block_bytes, filt)
    # the slot is honoured: without it the decode gives the differences, not the tensor
    rec = block.compress_tensor(stamps.to(dev), filter=filt, delta=True)
    plain = block.compress_tensor(stamps.to(dev), filter=filt)
    assert plain.delta is False
    if filt == "bitshuffle":
        assert rec.compressed_bytes < 0.8 * plain.compressed_bytes
    rec.delta = False
    assert not torch.equal(block.decompress_tensor(rec).cpu(), stamps)
    with pytest.raises(ValueError):
        block.compress_tensor(stamps.to(dev), delta=1)
    # the device forms, block by block
    x = stamps[:2048].to(dev).view(torch.uint8)
    off, ln = torch.tensor([0, 8192]), torch.tensor([8192, 8192])
    y, y_off = block.filter_blocks_device(x, off, ln, filt, 8, delta=True)
    back, _ = block.filter_blocks_device(y, y_off, ln, filt, 8, inverse=True, delta=True)
    assert torch.equal(back, x)
    host = x.cpu().numpy()
    assert (y.cpu().numpy()[:8192] == D.forward(host[:8192], block.FILTERS[filt], 8)).all()
