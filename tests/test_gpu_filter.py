"""GPU tests of the typed batches (lz4_filter.hip behind lz4flex_filter_batch, lz4flex_compress_batch_typed, lz4flex_decompress_batch_typed
and the tensor forms of lz4_flex_amd.block): the kernels against the numpy model of tests/filter_model.py at every length and alignment
at which they change path, canaries around everything they write; the typed codec calls against the plain ones over model-filtered
bytes and against the oracle."""
import ctypes as C

import numpy as np
import pytest

import filter_model as M
import oracle_api as O
import packed_cases as P

pytestmark = pytest.mark.gpu

CANARY = 0xC5
GUARD = 32                      # canary bytes in front of and behind every output slot
TILE = 1024                     # elements per (block, tile) work item (lz4_device.h FILTER_TILE_ELEMS)
FILTER_E = [(f, e) for f in (M.SHUFFLE, M.BITSHUFFLE) for e in M.ELEMS]
E_OUTPUT_TOO_SMALL = 1


@pytest.fixture(scope="module")
def lib():
    from lz4_flex_amd import _lib
    lib = _lib.load()
    if lib.lz4flex_device_count() < 1:
        pytest.fail("GPU tests need a device: " + _lib.last_error())
    return lib


@pytest.fixture
def ctx(lib):
    c = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(c), -1) == 0
    yield c
    lib.lz4flex_ctx_destroy(c)


def _ptr(a):
    if a is None:
        return None
    return C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else C.c_void_p(a.data_ptr())


class Batch:
    """arrays of one call in one memory kind: put() hands a numpy array over (device: a copy on the GPU), get() reads it back"""

    def __init__(self, mem, big=False):
        from lz4_flex_amd import _lib
        self.device = mem == "device"
        self.kind = (_lib.MEM_DEVICE if self.device else _lib.MEM_HOST) | (_lib.MEM_BIG_BLOCKS if big else 0)
        self.stream = None
        if self.device:
            import torch
            self.stream = C.c_void_p(torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream)

    def put(self, a):
        return P._dev(a) if self.device else a.copy()

    def get(self, x, dtype):
        if not self.device:
            return x
        import torch
        torch.cuda.synchronize()
        return P._host(x, dtype)


def lay_out(lens, res, guard):
    """offsets of slots of lens[i] bytes, slot i at residue res[i] mod 16, `guard` bytes free on both sides of each: (off, total)"""
    off, at = [], 0
    for ln, r in zip(lens, res):
        at = (at + guard + 15) // 16 * 16 + r
        off.append(at)
        at += ln + guard
    return np.array(off, np.uint64), at + 16


def run_filter(lib, ctx, mem, blocks, in_res, out_res, filt, E, inv):
    """lz4flex_filter_batch over `blocks` (uint8 arrays); returns the whole output buffer and the offsets of its slots"""
    from lz4_flex_amd import _lib
    lens = np.array([b.size for b in blocks], np.uint32)
    in_off, in_total = lay_out(lens, in_res, 0)
    out_off, out_total = lay_out(lens, out_res, GUARD)
    buf = np.full(in_total, 0x3C, np.uint8)
    for b, o in zip(blocks, in_off):
        buf[int(o):int(o) + b.size] = b
    m = Batch(mem)
    out = m.put(np.full(out_total, CANARY, np.uint8))
    keep = [m.put(buf), m.put(in_off), m.put(lens), m.put(out_off)]
    rc = lib.lz4flex_filter_batch(ctx, _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]), len(blocks), _ptr(out), _ptr(keep[3]), filt, E, int(inv),
                                  m.kind, m.stream)
    assert rc == 0, (rc, _lib.last_error())
    return m.get(out, np.uint8), out_off, out_total


def check_filter(lib, ctx, mem, blocks, in_res, out_res, filt, E, inv, wants, what):
    got, out_off, out_total = run_filter(lib, ctx, mem, blocks, in_res, out_res, filt, E, inv)
    image = np.full(out_total, CANARY, np.uint8)
    for w, o in zip(wants, out_off):
        image[int(o):int(o) + w.size] = w
    bad = np.nonzero(got != image)[0]
    if bad.size:
        i = int(np.searchsorted(out_off, bad[0], side="right")) - 1
        raise AssertionError("%s: %d bytes differ from the model / the canary, first at %d (block %d of %d bytes, slot at %d)"
                             % (what, bad.size, bad[0], i, blocks[max(i, 0)].size, out_off[max(i, 0)]))


def edge_lengths(E):
    """the lengths of the issue, and two at which a block of several tiles takes the wide path with a head, a partial tile and a tail:
    W1 = 29 chunks of 128 elements (bit planes of a multiple of 16 bytes), W2 = 131 lanes of 16 elements (byte planes of a multiple of 16
    bytes whose bit planes are not)"""
    return [0, 1, E - 1, E, 8 * E - 1, 8 * E, 8 * E + 1, 63 * E, 64 * E, 64 * E + 3, 1024 * E - 1, 1024 * E + 1, (TILE - 1) * E, TILE * E,
            (TILE + 1) * E, 65536, 65537, (1 << 20) + 13, 128 * E * 29 + E - 1, 16 * E * 131 + E - 1]


@pytest.fixture(scope="module")
def edge_batches():
    """per E: the blocks (each length three times: both offsets aligned, and two pairs of residues that run through 0 .. 15 independently),
    and per filter the model's forward transform of each"""
    rnd = np.random.default_rng(2020)
    res = {}
    for E in M.ELEMS:
        lens = edge_lengths(E)
        blocks, in_res, out_res = [], [], []
        for r in range(3):
            for k, ln in enumerate(lens):
                blocks.append(rnd.integers(0, 256, ln, dtype=np.uint8))
                in_res.append(0 if r == 0 else (k + 5 * r) % 16)
                out_res.append(0 if r == 0 else (7 * k + 3 * r) % 16)
        assert set(in_res) == set(range(16)) and set(out_res) == set(range(16))
        res[E] = (blocks, in_res, out_res, {f: [M.forward(b, f, E) for b in blocks] for f in (M.SHUFFLE, M.BITSHUFFLE)})
    return res


@pytest.mark.parametrize("inv", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("filt,E", FILTER_E)
def test_filter_batch_is_the_model(lib, ctx, edge_batches, filt, E, inv):
    blocks, in_res, out_res, fwd = edge_batches[E]
    src, want = (fwd[filt], blocks) if inv else (blocks, fwd[filt])
    for bytewise in (0, 1):
        assert lib.lz4flex_set_tuning(ctx, b"filter_bytewise", bytewise) == 0
        check_filter(lib, ctx, "device", src, in_res, out_res, filt, E, inv, want, "filter %d E %d inverse %d bytewise %d" % (filt, E, inv, bytewise))
    # a subset through host memory (every length once, the residue pairs of the second round)
    n = len(blocks) // 3
    sel = slice(n, 2 * n)
    assert lib.lz4flex_set_tuning(ctx, b"filter_bytewise", 0) == 0
    check_filter(lib, ctx, "host", src[sel], in_res[sel], out_res[sel], filt, E, inv, want[sel], "host filter %d E %d inverse %d" % (filt, E, inv))


@pytest.mark.parametrize("filt,E", FILTER_E)
def test_grid_shapes(lib, ctx, filt, E):
    """many small blocks (a wavefront takes several), one long block (every wavefront takes its tiles): 8 MiB + 5 as the issue has it --
    for most E a block whose planes cannot be aligned together -- and 8 MiB, which takes the wide path"""
    rnd = np.random.default_rng(100 * filt + E)
    small = rnd.integers(0, 256, (20000, 48), dtype=np.uint8)
    shapes = [("20 000 x 48", [row for row in small], [k % 16 for k in range(20000)], [(3 * k + 1) % 16 for k in range(20000)])]
    for ln in ((8 << 20) + 5, 8 << 20):
        shapes.append(("1 x %d" % ln, [rnd.integers(0, 256, ln, dtype=np.uint8)], [0], [0]))
    for what, blocks, in_res, out_res in shapes:
        fwd = [M.forward(b, filt, E) for b in blocks]
        check_filter(lib, ctx, "device", blocks, in_res, out_res, filt, E, False, fwd, "%s filter %d E %d forward" % (what, filt, E))
        check_filter(lib, ctx, "device", fwd, in_res, out_res, filt, E, True, blocks, "%s filter %d E %d inverse" % (what, filt, E))


def test_filter_none_is_a_copy(lib, ctx, edge_batches):
    blocks, in_res, out_res, _fwd = edge_batches[2]
    for inv in (False, True):
        check_filter(lib, ctx, "device", blocks, in_res, out_res, M.NONE, 4, inv, blocks, "copy")
    check_filter(lib, ctx, "host", blocks[:20], in_res[:20], out_res[:20], M.NONE, 1, False, blocks[:20], "host copy")


# ---- the typed codec calls -------------------------------------------------------------------------------------------------------
def numeric_blocks(E, seed):
    """about 40 blocks of numeric data of mixed lengths (0 ... 70 000 bytes and one of 200 000), not all multiples of E or of 8 E: bf16
    weights, int64 timestamps, a smooth fp32 signal with a little noise, ids below 5 000, random bytes"""
    rnd = np.random.default_rng(seed)
    t = np.arange(60000, dtype=np.float64)
    sources = [M.bf16_weights(240000, seed), M.int64_timestamps(240000, seed + 1),
               (np.sin(t / 500.0) + rnd.standard_normal(60000) * 1e-3).astype(np.float32).view(np.uint8),
               rnd.integers(0, 5000, 60000).astype(np.int32).view(np.uint8), rnd.integers(0, 256, 240000, dtype=np.uint8)]
    lens = [0, 1, E, 8 * E + 1, 12, 13, 14, 65536, 65535, 70000, 200000, 4096, 4097, 1024 * E, 128 * E * 5 + 3] + \
        [int(v) for v in rnd.integers(0, 70000, 16)] + [int(v) for v in rnd.integers(0, 600, 9)]
    blocks = []
    for k, ln in enumerate(lens):
        s = sources[k % len(sources)]
        a = int(rnd.integers(0, (s.size - ln) // 8 + 1)) * 8
        blocks.append(s[a:a + ln].copy())
    return blocks


def run_compress(lib, ctx, mem, name, blocks, caps, filt=None, E=None):
    """lz4flex_compress_batch (name "plain") or lz4flex_compress_batch_typed over `blocks` into canary-guarded slots of caps[i] bytes"""
    from lz4_flex_amd import _lib
    n = len(blocks)
    lens = np.array([b.size for b in blocks], np.uint32)
    in_off, in_total = lay_out(lens, [(5 * k) % 16 for k in range(n)], 0)
    out_off, out_total = lay_out(caps, [(3 * k) % 16 for k in range(n)], GUARD)
    buf = np.full(in_total, 0x3C, np.uint8)
    for b, o in zip(blocks, in_off):
        buf[int(o):int(o) + b.size] = b
    m = Batch(mem, big=mem == "device")
    out, out_len, status = m.put(np.full(out_total, CANARY, np.uint8)), m.put(np.full(n, 0xA5A5A5A5, np.uint32)), m.put(np.full(n, 0x5A5A5A5A, np.int32))
    keep = [m.put(buf), m.put(in_off), m.put(lens), m.put(out_off), m.put(np.asarray(caps, np.uint32))]
    head = [ctx, _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2])]
    slots = [_ptr(out), _ptr(keep[3]), _ptr(keep[4]), _ptr(out_len), _ptr(status)]
    if name == "plain":
        rc = lib.lz4flex_compress_batch(*head, None, n, *slots, m.kind, m.stream)
    else:
        tmp = m.put(np.full(in_total, 0x77, np.uint8)) if m.device and filt != M.NONE else None
        rc = lib.lz4flex_compress_batch_typed(*head, n, *slots, filt, E, _ptr(tmp), _ptr(keep[1]) if tmp is not None else None, m.kind, m.stream)
    assert rc == 0, (name, rc, _lib.last_error())
    return dict(out=m.get(out, np.uint8), out_len=m.get(out_len, np.uint32), status=m.get(status, np.int32), out_off=out_off, caps=caps)


def same_compress_results(got, want, what):
    assert (got["status"] == want["status"]).all(), (what, np.nonzero(got["status"] != want["status"])[0][:4])
    assert (got["out_len"] == want["out_len"]).all(), (what, np.nonzero(got["out_len"] != want["out_len"])[0][:4])
    a, b = got["out"].copy(), want["out"].copy()
    for o, cap, st in zip(got["out_off"], got["caps"], got["status"]):
        if st != 0:                                      # (what a block that did not fit left in its own slot is nobody's contract)
            a[int(o):int(o) + int(cap)] = b[int(o):int(o) + int(cap)] = 0
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, "%s: %d bytes of the output differ, first at %d" % (what, bad.size, bad[0])


@pytest.mark.parametrize("mode", [0, 1], ids=["fast", "exact"])
@pytest.mark.parametrize("mem,filt,E", [("device", M.SHUFFLE, 2), ("device", M.SHUFFLE, 8), ("device", M.BITSHUFFLE, 2), ("device", M.BITSHUFFLE, 4),
                                        ("host", M.BITSHUFFLE, 2), ("host", M.SHUFFLE, 4)])
def test_typed_compress_is_compress_batch_of_the_filtered_bytes(lib, ctx, mem, filt, E, mode):
    blocks = numeric_blocks(E, 31 * E + filt)
    n = len(blocks)
    assert 35 <= n <= 45
    filtered = [M.forward(b, filt, E) for b in blocks]
    caps = [O.max_out(b.size) for b in blocks]
    short = 9                                            # 70 000 random bytes with a slot below what they need
    assert blocks[short].size == 70000
    caps[short] = blocks[short].size // 2
    assert lib.lz4flex_set_tuning(ctx, b"compress_mode", mode) == 0
    want = run_compress(lib, ctx, mem, "plain", filtered, caps)
    got = run_compress(lib, ctx, mem, "typed", blocks, caps, filt, E)
    same_compress_results(got, want, "typed compress %s filter %d E %d mode %d" % (mem, filt, E, mode))
    assert got["status"][short] == E_OUTPUT_TOO_SMALL and (np.delete(got["status"], short) == 0).all()
    # everything outside the slots is canary
    image = np.full(got["out"].size, CANARY, np.uint8)
    for o, cap in zip(got["out_off"], caps):
        image[int(o):int(o) + cap] = got["out"][int(o):int(o) + cap]
    assert (got["out"] == image).all()
    for i, (b, f) in enumerate(zip(blocks, filtered)):
        if i == short:
            continue
        o, ln = int(got["out_off"][i]), int(got["out_len"][i])
        comp = got["out"][o:o + ln].tobytes()
        if mode == 1:
            assert comp == O.compress(f.tobytes()), (i, b.size)
        st, back = O.decompress(comp, b.size)
        assert st == "ok" and (M.inverse(np.frombuffer(back, np.uint8), filt, E) == b).all(), (i, b.size, st)


def run_decompress(lib, ctx, mem, name, comps, caps, filt=None, E=None):
    from lz4_flex_amd import _lib
    n = len(comps)
    buf, in_off, lens = P.pack(comps, odd=True)
    out_off, out_total = lay_out(caps, [(3 * k) % 16 for k in range(n)], GUARD)
    m = Batch(mem, big=mem == "device")
    out, out_len, status = m.put(np.full(out_total, CANARY, np.uint8)), m.put(np.full(n, 0xA5A5A5A5, np.uint32)), m.put(np.full(n, 0x5A5A5A5A, np.int32))
    detail = m.put(np.full(2 * n, 0xA5A5A5A5A5A5A5A5, np.uint64))
    keep = [m.put(buf), m.put(in_off), m.put(lens), m.put(out_off), m.put(np.asarray(caps, np.uint32))]
    args = [ctx, _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]), n, _ptr(out), _ptr(keep[3]), _ptr(keep[4]), _ptr(out_len), _ptr(status), _ptr(detail)]
    if name == "plain":
        rc = lib.lz4flex_decompress_batch(*args, m.kind, m.stream)
    else:
        tmp = m.put(np.full(out_total, 0x77, np.uint8)) if m.device and filt != M.NONE else None
        rc = lib.lz4flex_decompress_batch_typed(*args, filt, E, _ptr(tmp), _ptr(keep[3]) if tmp is not None else None, m.kind, m.stream)
    assert rc == 0, (name, rc, _lib.last_error())
    return dict(out=m.get(out, np.uint8), out_len=m.get(out_len, np.uint32), status=m.get(status, np.int32),
                detail=m.get(detail, np.uint64).reshape(n, 2), out_off=out_off)


def same_decode_results(got, want, mem):
    """status, out_len and detail are lz4flex_decompress_batch's.  The decoders write the detail of an OutputTooSmall block alone: a
    DEVICE call leaves the other blocks' words as the caller filled them, a HOST call hands back whatever its staging memory held there --
    those words are compared where they are defined"""
    for k in ("status", "out_len"):
        assert (got[k] == want[k]).all(), (k, np.nonzero(got[k] != want[k])[0][:4])
    rows = got["status"] == E_OUTPUT_TOO_SMALL if mem == "host" else np.ones(len(got["status"]), bool)
    assert (got["detail"][rows] == want["detail"][rows]).all(), ("detail", got["detail"][rows][:2], want["detail"][rows][:2])


@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("filt,E", FILTER_E)
def test_typed_decompress_gives_the_numbers_back(lib, ctx, mem, filt, E):
    blocks = numeric_blocks(E, 17 * E + filt)
    if mem == "host":
        blocks = blocks[:16]
    n = len(blocks)
    comps = [O.compress(M.forward(b, filt, E).tobytes()) for b in blocks]
    caps = [b.size + (7 if k % 4 == 1 else 0) for k, b in enumerate(blocks)]      # some slots larger than the block
    damaged, short = 7, 9
    assert blocks[damaged].size == 65536 and blocks[short].size > 1000
    comps[damaged] = comps[damaged][:len(comps[damaged]) // 2] + bytes(3)      # cut in the middle: an offset of zero, or literals that run out
    caps[short] = blocks[short].size - 1
    want = run_decompress(lib, ctx, mem, "plain", comps, caps)
    got = run_decompress(lib, ctx, mem, "typed", comps, caps, filt, E)
    same_decode_results(got, want, mem)
    assert got["status"][damaged] != 0 and got["status"][short] == E_OUTPUT_TOO_SMALL and (np.delete(got["status"], [damaged, short]) == 0).all()
    # the good blocks are the inputs, the failed blocks' slots and everything between the slots are canary
    image = np.full(got["out"].size, CANARY, np.uint8)
    for i, (b, o) in enumerate(zip(blocks, got["out_off"])):
        if i not in (damaged, short):
            image[int(o):int(o) + b.size] = b
    wrong = np.nonzero(got["out"] != image)[0]
    assert wrong.size == 0, "typed decompress %s filter %d E %d: %d bytes differ, first at %d" % (mem, filt, E, wrong.size, wrong[0])


@pytest.mark.parametrize("mem", ["device", "host"])
def test_filter_none_is_the_plain_entry(lib, ctx, mem):
    blocks = numeric_blocks(4, 5)
    caps = [O.max_out(b.size) for b in blocks]
    for mode in (0, 1):
        assert lib.lz4flex_set_tuning(ctx, b"compress_mode", mode) == 0
        want = run_compress(lib, ctx, mem, "plain", blocks, caps)
        got = run_compress(lib, ctx, mem, "typed", blocks, caps, M.NONE, 4)
        same_compress_results(got, want, "FILTER_NONE compress %s mode %d" % (mem, mode))
        assert (got["status"] == 0).all()
    comps = [O.compress(b.tobytes()) for b in blocks]
    sizes = [b.size for b in blocks]
    sizes[9] -= 1
    want = run_decompress(lib, ctx, mem, "plain", comps, sizes)
    got = run_decompress(lib, ctx, mem, "typed", comps, sizes, M.NONE, 8)
    same_decode_results(got, want, mem)
    ok = np.nonzero(got["status"] == 0)[0]
    assert ok.size == len(blocks) - 1
    for i in ok:
        o = int(got["out_off"][i])
        assert (got["out"][o:o + blocks[i].size] == blocks[i]).all(), i


# ---- tensors -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", ["bitshuffle", "shuffle", "none"])
def test_tensor_round_trip_is_bitwise(lib, filt):
    import torch
    from lz4_flex_amd import block
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(9)
    n = 200003                                          # the byte sizes are no multiples of block_bytes or of 8 E
    tensors = [(torch.randn(n, generator=g) * 0.02).to(torch.bfloat16), torch.randn(n, generator=g) * 0.02,
               torch.cumsum(torch.randint(900, 1100, (n,), generator=g), 0) + 1_700_000_000_000,
               torch.randint(0, 256, (n,), generator=g).to(torch.uint8), torch.randn(7, 11, 13, generator=g).to(torch.float16)]
    assert [t.dtype for t in tensors[:4]] == [torch.bfloat16, torch.float32, torch.int64, torch.uint8]
    for t in tensors:
        for block_bytes in (65536, 4096):
            rec = block.compress_tensor(t.to(dev), block_bytes=block_bytes, filter=filt)
            assert rec.shape == tuple(t.shape) and rec.dtype == t.dtype and rec.block_bytes == block_bytes and rec.filter == block.FILTERS[filt]
            n_blocks = (t.numel() * t.element_size() + block_bytes - 1) // block_bytes
            assert rec.offsets.numel() == n_blocks and rec.lengths.numel() == n_blocks and rec.compressed_bytes == int(rec.lengths.sum())
            back = block.decompress_tensor(rec)
            assert back.dtype == t.dtype and back.shape == t.shape and back.device.type == "cuda"
            assert torch.equal(back.cpu().view(torch.uint8), t.view(torch.uint8)), (t.dtype, block_bytes, filt)
    # the reason for the feature, on the device: bit-shuffled bf16 weights are smaller than raw ones
    if filt == "bitshuffle":
        w = tensors[0].to(dev)
        assert block.compress_tensor(w, filter="bitshuffle").compressed_bytes < 0.9 * block.compress_tensor(w, filter="none").compressed_bytes


def test_tensor_forms_refuse_what_they_cannot_take(lib):
    import torch
    from lz4_flex_amd import block
    dev = torch.device("cuda", 0)
    with pytest.raises(ValueError):
        block.compress_tensor(torch.zeros(64, dtype=torch.complex128, device=dev))
    with pytest.raises(ValueError):
        block.compress_tensor(torch.zeros(64, 64, device=dev).t())
    with pytest.raises(ValueError):
        block.compress_tensor(torch.zeros(64, device=dev), block_bytes=4098)
    with pytest.raises(ValueError):
        block.compress_tensor(torch.zeros(64, device=dev), filter="delta")
    empty = block.compress_tensor(torch.zeros(0, 3, device=dev))
    assert empty.compressed_bytes == 0 and block.decompress_tensor(empty).shape == (0, 3)
    # the device forms, block by block
    x = torch.arange(4096, dtype=torch.int32, device=dev).view(torch.uint8)
    off, ln = torch.tensor([0, 8192]), torch.tensor([8192, 8192])
    y, y_off = block.filter_blocks_device(x, off, ln, "shuffle", 4)
    back, _ = block.filter_blocks_device(y, y_off, ln, "shuffle", 4, inverse=True)
    assert torch.equal(back, x)
    host = x.cpu().numpy()
    assert (y.cpu().numpy()[:8192] == M.shuffle(host[:8192], 4)).all() and (y.cpu().numpy()[8192:] == M.shuffle(host[8192:], 4)).all()
