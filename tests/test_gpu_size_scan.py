"""GPU tests of the decompressed-size query (lz4flex_decompressed_size_batch, lz4_size_scan.hip): every status and size equals the
oracle's decompress_internal with an unbounded sink (tests/size_model.py is pinned to it on the CPU: test_size_scan_model.py), in both
passes ("size_scan_serial" 0 / 1), HOST and DEVICE; a block the query calls valid decodes with out_cap = its size on every decoder
configuration; decompress_blocks_device round-trips the benchmark's JSON batch with exactly sized output."""
import ctypes as C
import random

import numpy as np
import pytest

import corpus
import ext_cases
import oracle_api as O
import seq_blocks
import size_model as S

pytestmark = pytest.mark.gpu

CANARY_SIZE, CANARY_ST = 0xA5A5A5A5A5A5A5A5, 0x5A5A5A5A


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


def oracle_size(c, history=0):
    cap = 255 * len(c) + 64
    st, r = O.decompress(c, cap) if history == 0 else O.decompress_prefix(c, bytes(history), history + cap)
    if st == "ok":
        return 0, len(r)
    return {v: k for k, v in S.NAMES.items()}[st], 0


def pack(blocks, gap=0):
    offs, lens, at = [], [], 0
    for c in blocks:
        offs.append(at)
        lens.append(len(c))
        at += len(c) + gap
    buf = bytearray(max(at, 1))
    for o, c in zip(offs, blocks):
        buf[o:o + len(c)] = c
    return np.frombuffer(bytes(buf), np.uint8), np.array(offs, np.uint64), np.array(lens, np.uint32)


def scan(lib, ctx, blocks, history=None, mode="host", serial=0, extra=4):
    """(size, status) of every block through the C entry point; checks that the `extra` result slots behind n are untouched"""
    from lz4_flex_amd import _lib
    assert lib.lz4flex_set_tuning(ctx, b"size_scan_serial", serial) == 0
    buf, offs, lens = pack(blocks, gap=3)
    n = len(blocks)
    hist = None if history is None else np.ascontiguousarray(history, np.uint32)
    size = np.full(n + extra, CANARY_SIZE, np.uint64)
    st = np.full(n + extra, CANARY_ST, np.int32)
    if mode == "host":
        rc = lib.lz4flex_decompressed_size_batch(ctx, C.c_void_p(buf.ctypes.data), C.c_void_p(offs.ctypes.data), C.c_void_p(lens.ctypes.data), n,
                                                 None if hist is None else C.c_void_p(hist.ctypes.data), C.c_void_p(size.ctypes.data),
                                                 C.c_void_p(st.ctypes.data), _lib.MEM_HOST, None)
        assert rc == 0, _lib.last_error()
    else:
        import torch
        dev = torch.device("cuda", 0)
        t = {k: torch.from_numpy(np.array(v.view(np.int64) if v.dtype == np.uint64 else v.view(np.int32) if v.dtype == np.uint32 else v)).to(dev)
             for k, v in (("buf", buf), ("offs", offs), ("lens", lens), ("size", size), ("st", st))}
        th = None if hist is None else torch.from_numpy(hist.view(np.int32)).to(dev)
        stream = torch.cuda.current_stream(dev)
        rc = lib.lz4flex_decompressed_size_batch(ctx, C.c_void_p(t["buf"].data_ptr()), C.c_void_p(t["offs"].data_ptr()),
                                                 C.c_void_p(t["lens"].data_ptr()), n, None if th is None else C.c_void_p(th.data_ptr()),
                                                 C.c_void_p(t["size"].data_ptr()), C.c_void_p(t["st"].data_ptr()),
                                                 _lib.MEM_DEVICE | _lib.MEM_BIG_BLOCKS, C.c_void_p(stream.cuda_stream))
        assert rc == 0, _lib.last_error()
        stream.synchronize()
        size = t["size"].cpu().numpy().view(np.uint64)
        st = t["st"].cpu().numpy()
    assert (size[n:] == CANARY_SIZE).all() and (st[n:] == CANARY_ST).all(), "results written past n"
    return size[:n], st[:n]


def expect(size, st, want):
    got = [(int(s), int(z)) for s, z in zip(st, size)]
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, "%d of %d blocks differ, first: %s" % (len(bad), len(want), bad[:5])


@pytest.fixture(scope="module")
def adversarial():
    blocks = [c for c, _cap in corpus.adversarial_blocks()]
    return blocks, [oracle_size(c) for c in blocks]


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("serial", [0, 1])
def test_adversarial_corpus(lib, ctx, adversarial, mode, serial):
    blocks, want = adversarial
    size, st = scan(lib, ctx, blocks, mode=mode, serial=serial)
    expect(size, st, want)
    assert {s for s, _ in want} == {0, 2, 3, 4, 5}


@pytest.mark.parametrize("serial", [0, 1])
def test_hand_written_blocks(lib, ctx, serial):
    cases = S.writer_cases()
    blocks = [c for _n, c, _h in cases]
    hist = [h for _n, _c, h in cases]
    size, st = scan(lib, ctx, blocks, history=hist, serial=serial)
    expect(size, st, [oracle_size(c, h) for c, h in zip(blocks, hist)])


@pytest.mark.parametrize("mode", ["host", "device"])
def test_history(lib, ctx, mode):
    blocks, hist, with_h, without_h = [], [], [], []
    for p in ext_cases.PREFIX_LENS:
        prefix = ext_cases.prefix_bytes(p)
        for name, c, new in ext_cases.writer_blocks(prefix):
            blocks.append(c)
            hist.append(p)
            w = oracle_size(c, p)
            if new is not None:
                assert w == (0, len(new)), name
            with_h.append(w)
            without_h.append(oracle_size(c))
    size, st = scan(lib, ctx, blocks, history=hist, mode=mode)
    expect(size, st, with_h)
    size, st = scan(lib, ctx, blocks, mode=mode)
    expect(size, st, without_h)
    # blocks that reach into their prefix: valid behind it, OffsetOutOfBounds without it
    assert sum(1 for a, b in zip(with_h, without_h) if a[0] == 0 and b[0] == S.OFFSET_OUT_OF_BOUNDS) > 20


def exact_len_block(target, seed):
    """a valid block of exactly `target` compressed bytes: sequences, then a last literal run that fills it up"""
    from lz4_writer import Writer
    rnd = random.Random(seed)
    w = Writer(seed)
    w.seq(8, 3, 20)
    while len(w.comp) < target - 600:
        w.seq(rnd.randint(0, 30), rnd.randint(1, min(len(w.out), 3000)), rnd.randint(4, 300))
    r = target - len(w.comp)
    for lit in range(r, 0, -1):
        if 1 + (1 + (lit - 15) // 255 if lit >= 15 else 0) + lit == r:
            c, _ = w.end(lit)
            assert len(c) == target
            return c
    raise AssertionError(target)


def test_shapes(lib, ctx):
    T = 3840
    blocks = [b"", b"\x00", b"\x10", b"\x10a", b"\x00\x01", b"\x11a\x01\x00"]
    for t in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 7):
        c = exact_len_block(t, t)
        blocks += [c, c[:-1], c[:T], c[:T + 1], c[:T - 1], c + b"\x00"]
    for mode in ("host", "device"):
        for serial in (0, 1):
            size, st = scan(lib, ctx, blocks, mode=mode, serial=serial)
            expect(size, st, [oracle_size(c) for c in blocks])


@pytest.fixture(scope="module")
def walk_blocks():
    """the sequence decoder's own list: ((block, expected), ...) for every block whole, then for every block cut by 3 bytes"""
    named = seq_blocks.blocks()
    whole = [(c, (0, len(p))) for _name, c, p in named]
    cut = [(c[:-3], S.size(c[:-3])) for _name, c, _p in named]
    return [name for name, _c, _p in named], whole, cut


@pytest.mark.parametrize("serial", [0, 1])
def test_blocks_on_the_walks_boundaries(lib, ctx, walk_blocks, serial):
    """the size scan shares the decoder's tile walk (lz4_seq_walk.h): the blocks test_gpu_seq.py writes onto the walk's boundaries -- 6 000
    three-byte sequences, tile boundaries shifted by 0 .. 63, literal runs that jump over tiles, of 3 839 / 3 840 / 3 841 bytes, literals
    only -- give status 0 and len(plain); cut by 3 bytes, what size_model says.  One DEVICE batch per pass."""
    names, whole, cut = walk_blocks
    assert len(names) >= 150 and "6 000 three-byte sequences" in names and "literals only 0" in names
    size, st = scan(lib, ctx, [c for c, _w in whole + cut], mode="device", serial=serial)
    expect(size, st, [w for _c, w in whole + cut])


def test_large_blocks(lib, ctx):
    import torch
    from lz4_flex_amd import workloads
    plain = O.fixture_plain("compression_66k_JSON")
    j16 = workloads.json_tiles(plain, 16 << 20, phase=123).numpy().tobytes()
    log4 = workloads.log_stream(0, 4 << 20).numpy().tobytes()
    rnd = np.random.default_rng(3)
    noise = rnd.integers(0, 256, 4 << 20, dtype=np.uint8).tobytes()
    blocks = [O.compress(j16), O.c_compress(log4), O.compress(noise), O.compress(bytes(4 << 20)), O.compress(j16[:4 << 20])]
    want = [(0, len(j16)), (0, len(log4)), (0, len(noise)), (0, 4 << 20), (0, 4 << 20)]
    for mode in ("host", "device"):
        size, st = scan(lib, ctx, blocks, mode=mode)
        expect(size, st, want)
    size, st = scan(lib, ctx, blocks[1:], serial=1)
    expect(size, st, want[1:])
    # the same blocks cut short: errors the parallel pass hands to the serial one
    cut = [c[:len(c) // 2] for c in blocks]
    size, st = scan(lib, ctx, cut, mode="device")
    expect(size, st, [oracle_size(c) for c in cut])
    torch.cuda.synchronize()


def pool_blocks():
    """blocks from the GPU's two encoders, the oracle (lz4_flex's bytes) and C liblz4"""
    from lz4_flex_amd import block
    plain = O.fixture_plain("compression_66k_JSON") + O.fixture_plain("compression_65k")
    rnd = random.Random(11)
    out = []
    for k in range(24):
        a = rnd.randint(0, len(plain) - 9000)
        d = plain[a:a + rnd.choice((20, 300, 1000, 4000, 8192))]
        enc = (O.compress, O.c_compress, block.compress)[k % 3]
        out.append(enc(d))
    block.set_compress_mode("exact")
    try:
        out += [block.compress(plain[k * 5000:k * 5000 + 6000]) for k in range(4)]
    finally:
        block.set_compress_mode("fast")
    out += [out[0][:-1], out[1][:5], b""]
    return out


@pytest.mark.parametrize("n", [1, 640, 641, 14336, 14337, 16384])
def test_batch_sizes(lib, ctx, n):
    pool = pool_blocks()
    want_pool = [oracle_size(c) for c in pool]
    idx = [(i * 7) % len(pool) for i in range(n)]
    blocks = [pool[i] for i in idx]
    for mode in ("host", "device"):
        size, st = scan(lib, ctx, blocks, mode=mode)
        expect(size, st, [want_pool[i] for i in idx])


def test_valid_blocks_decode_with_exact_capacity(lib, adversarial):
    """the key property: status 0 and size S => decode with out_cap = S on every decoder configuration gives status 0, out_len S and
    the oracle's bytes"""
    from lz4_flex_amd import block
    blocks = [c for c, (s, _z) in zip(*adversarial) if s == 0]
    blocks += [c for _n, c, h in S.writer_cases() if h == 0 and oracle_size(c)[0] == 0]
    blocks += pool_blocks()
    blocks = [c for c in blocks if oracle_size(c)[0] == 0]
    c0 = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(c0), -1) == 0
    try:
        size, st = scan(lib, c0, blocks)
    finally:
        lib.lz4flex_ctx_destroy(c0)
    assert (st == 0).all()
    plains = [O.decompress(c, int(z))[1] for c, z in zip(blocks, size)]
    buf, offs, lens = pack(blocks)
    out_off = np.concatenate([[0], np.cumsum(size.astype(np.int64))[:-1]]).astype(np.uint64)
    cap = size.astype(np.uint32)
    i, configs = 0, []
    while True:
        v = lib.lz4flex_get_tuning(None, b"decoder_config_%d" % i)
        if v < 0:
            break
        configs.append(v)
        i += 1
    assert configs
    for cfg in configs:
        variant, par = divmod(cfg, 1000)
        c = C.c_void_p()
        assert lib.lz4flex_ctx_create(C.byref(c), -1) == 0
        try:
            assert lib.lz4flex_set_tuning(c, b"decompress_variant", variant) == 0
            if variant == 1:
                assert lib.lz4flex_set_tuning(c, b"decompress_lanes", par) == 0
            if variant == 4:
                assert lib.lz4flex_set_tuning(c, b"decompress_blocks_per_wg", par) == 0
            out = np.zeros(int(size.sum()) + 64, np.uint8)
            out_len, st2, _det = block.decompress_batch(buf, offs, lens, out, out_off, cap, ctx=c)
        finally:
            lib.lz4flex_ctx_destroy(c)
        assert (st2 == 0).all(), (cfg, np.nonzero(st2)[0][:5], st2[st2 != 0][:5])
        assert (out_len == cap).all(), cfg
        for k, p in enumerate(plains):
            o = int(out_off[k])
            assert out[o:o + len(p)].tobytes() == p, (cfg, k)


def test_decompress_blocks_device_bench_workload():
    """config 2 of bench.py: workloads.json_tiles over the compression_66k_JSON fixture, 16 384 blocks of 64 KiB, the default encoder"""
    import torch
    from lz4_flex_amd import block, sharded, workloads
    dev = torch.device("cuda", 0)
    plain = O.fixture_plain("compression_66k_JSON")
    n, bs = 16384, 65536
    src = workloads.json_tiles(plain, n * bs, device=dev)
    comp, comp_off, comp_len, _in_len = sharded.compress_blocks_device(src, bs, np.zeros(n, np.uint32))
    out, out_off, out_len, status = block.decompress_blocks_device(comp, comp_off, comp_len)
    assert out.numel() == n * bs
    assert int((status != 0).sum()) == 0
    assert bool((out_len == bs).all()) and bool((out_off == torch.arange(n, device=dev, dtype=torch.int64) * bs).all())
    assert torch.equal(out, src)
    # a failed block: its status, an empty slot; the others are unaffected
    bad_len = comp_len.clone()
    bad_len[5] = 3
    out, out_off, out_len, status = block.decompress_blocks_device(comp, comp_off, bad_len)
    st = status.cpu().numpy()
    assert st[5] != 0 and (np.delete(st, 5) == 0).all()
    assert int(out_len[5]) == 0 and out.numel() == (n - 1) * bs
    assert torch.equal(out[:5 * bs], src[:5 * bs]) and torch.equal(out[5 * bs:], src[6 * bs:])
