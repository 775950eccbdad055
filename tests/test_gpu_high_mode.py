"""GPU (-m gpu): compress_mode 2 ("high", lz4_compress_high.hip) through the C ABI.  The kernel must reproduce the scalar definition
(tests/sim/high_encoder_model.c) byte for byte at every depth, in every memory kind and through every entry that encodes independent
blocks without a dictionary; every other entry gives compress_mode 0's bytes under mode 2."""
import ctypes as C
import random

import numpy as np
import pytest

import hc_model as H
import oracle_api as O

pytestmark = pytest.mark.gpu

DEPTHS = (1, 4, 16, 64)
LENGTHS = (0, 1, 4, 11, 12, 13, 14, 17, 63, 64, 65, 4095, 4096, 32767, 32768, 32769, 65535, 65536, 65537, 98303, 98304, 98305, 66675, 200000)
KINDS = ("json", "text", "ab", "zeros", "period256", "runs", "random")
CANARY = 16


def content(kind, n, rnd):
    if kind == "json":
        return (O.fixture_plain("compression_66k_JSON") * 4)[:n]
    if kind == "text":
        return (O.fixture_plain("compression_65k") * 4)[:n]
    if kind == "ab":
        return bytes(rnd.choice(b"ab") for _ in range(n))
    if kind == "zeros":
        return bytes(n)
    if kind == "period256":
        return (bytes(range(256)) * (n // 256 + 1))[:n]
    if kind == "runs":
        out = bytearray()
        while len(out) < n:
            out += bytes([rnd.getrandbits(8)]) * rnd.randint(1, 700)
        return bytes(out[:n])
    return bytes(rnd.getrandbits(8) for _ in range(n))


_batch1 = []


def batch1():
    """every length with three of the seven contents, every content at every class of lengths: 72 blocks"""
    if not _batch1:
        rnd = random.Random(2024)
        for i, n in enumerate(LENGTHS):
            for kind in (("json", "zeros", "runs") if n == 200000 else [KINDS[(i + 3 * k) % 7] for k in range(3)]):
                _batch1.append(content(kind, n, rnd))
    return _batch1


_model = {}


def model(data, depth):
    key = (data, depth)
    if key not in _model:
        _model[key] = H.compress(data, depth)
    return _model[key]


@pytest.fixture(scope="module")
def env():
    from lz4_flex_amd import _lib
    lib = _lib.load()
    assert lib.lz4flex_device_count() >= 1
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
    assert lib.lz4flex_set_tuning(ctx, b"compress_mode", 2) == 0
    yield lib, ctx
    lib.lz4flex_ctx_destroy(ctx)


def layout(blocks, caps=None):
    """unaligned block starts; output slots of `caps` (default: the bound) with CANARY bytes in front of and behind each"""
    in_len = np.array([len(b) for b in blocks], dtype=np.uint32)
    in_off = np.zeros(len(blocks), dtype=np.uint64)
    in_off[1:] = np.cumsum(in_len.astype(np.uint64) + 3)[:-1]
    buf = np.zeros(int(in_off[-1] + in_len[-1]) + 64, dtype=np.uint8)
    for b, o in zip(blocks, in_off):
        buf[int(o):int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    cap = np.array([O.max_out(len(b)) for b in blocks] if caps is None else caps, dtype=np.uint32)
    out_off = np.zeros(len(blocks), dtype=np.uint64)
    out_off[:] = np.cumsum(cap.astype(np.uint64) + CANARY) - cap + 0
    out = np.full(int(out_off[-1] + cap[-1]) + CANARY, 0xEE, dtype=np.uint8)
    return buf, in_off, in_len, out, out_off, cap


def run_batch(lib, ctx, blocks, mem, caps=None, flags=None):
    """lz4flex_compress_batch over `blocks` in host or device memory: (the whole output buffer, out_off, out_len, status)"""
    from lz4_flex_amd import _lib as L
    buf, in_off, in_len, out, out_off, cap = layout(blocks, caps)
    n = len(blocks)
    fl = None if flags is None else np.array(flags, dtype=np.uint32)
    if mem & L.MEM_DEVICE:
        import torch
        dev = torch.device("cuda", 0)
        tt = lambda a, dt: torch.from_numpy(a.view(dt)).to(dev)      # noqa: E731
        d_in, d_out = torch.from_numpy(buf).to(dev), torch.from_numpy(out).to(dev)
        d = [tt(in_off, np.int64), tt(in_len, np.int32), tt(out_off, np.int64), tt(cap, np.int32)]
        d_fl = None if fl is None else tt(fl, np.int32)
        d_len = torch.zeros(n, dtype=torch.int32, device=dev)
        d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
        p = lambda x: None if x is None else C.c_void_p(x.data_ptr())      # noqa: E731
        rc = lib.lz4flex_compress_batch(ctx, p(d_in), p(d[0]), p(d[1]), p(d_fl), n, p(d_out), p(d[2]), p(d[3]), p(d_len), p(d_st), mem, None)
        assert rc == 0, L.last_error()
        torch.cuda.synchronize()
        return d_out.cpu().numpy(), out_off, d_len.cpu().numpy().view(np.uint32), d_st.cpu().numpy()
    out_len, st = np.zeros(n, dtype=np.uint32), np.full(n, -1, dtype=np.int32)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)      # noqa: E731
    rc = lib.lz4flex_compress_batch(ctx, p(buf), p(in_off), p(in_len), p(fl), n, p(out), p(out_off), p(cap), p(out_len), p(st), mem, None)
    assert rc == 0, L.last_error()
    return out, out_off, out_len, st


def check_against_model(blocks, depth, out, out_off, out_len, st, refused=()):
    """every slot holds the model's bytes (a refused one: nothing) and every byte outside the blocks' bytes is untouched"""
    want = np.full(out.size, 0xEE, dtype=np.uint8)
    for k, b in enumerate(blocks):
        if k in refused:
            assert (int(st[k]), int(out_len[k])) == (1, 0), k      # LZ4FLEX_E_OUTPUT_TOO_SMALL
            continue
        m = model(b, depth)
        assert int(st[k]) == 0 and int(out_len[k]) == len(m), (k, len(b), int(st[k]), int(out_len[k]), len(m))
        want[int(out_off[k]):int(out_off[k]) + len(m)] = np.frombuffer(m, dtype=np.uint8)
    bad = np.flatnonzero(want != out)
    if bad.size:
        k = int(np.searchsorted(out_off, bad[0], side="right")) - 1
        raise AssertionError("first difference at output byte %d: block %d (length %d), byte %d of its slot" % (bad[0], k, len(blocks[k]), bad[0] - int(out_off[k])))


@pytest.mark.parametrize("mem", ["host", "device", "device_big"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_kernel_equals_model(env, depth, mem):
    from lz4_flex_amd import _lib as L
    lib, ctx = env
    blocks = batch1()
    assert lib.lz4flex_set_tuning(ctx, b"compress_depth", depth) == 0
    kind = {"host": L.MEM_HOST, "device": L.MEM_DEVICE, "device_big": L.MEM_DEVICE | L.MEM_BIG_BLOCKS}[mem]
    out, out_off, out_len, st = run_batch(lib, ctx, blocks, kind)
    check_against_model(blocks, depth, out, out_off, out_len, st)
    if mem == "host":
        for k, b in enumerate(blocks):
            got = bytes(out[int(out_off[k]):int(out_off[k]) + int(out_len[k])])
            assert O.decompress(got, len(b)) == ("ok", b), k
            if b:
                assert O.c_decompress(got, len(b)) == b, k


def log_blocks(lib):
    from lz4_flex_amd import workloads
    n = 2 * lib.lz4flex_get_tuning(None, b"compress_workgroups") + 3
    rnd = random.Random(7)
    log = bytes(workloads.log_stream(0, 1 << 20).numpy())
    out = []
    for _ in range(n):
        ln = rnd.randint(1024, 3072)
        at = rnd.randrange(len(log) - ln)
        out.append(log[at:at + ln])
    return out


def test_more_blocks_than_workgroups(env):
    from lz4_flex_amd import _lib as L
    lib, ctx = env
    assert lib.lz4flex_set_tuning(ctx, b"compress_depth", 16) == 0
    blocks = log_blocks(lib)
    refused = set(range(6, len(blocks), 7))
    caps = [O.max_out(len(b)) - (1 if k in refused else 0) for k, b in enumerate(blocks)]
    out, out_off, out_len, st = run_batch(lib, ctx, blocks, L.MEM_DEVICE, caps=caps)
    check_against_model(blocks, 16, out, out_off, out_len, st, refused)


def test_bytes_depend_on_block_and_depth_only(env):
    from lz4_flex_amd import _lib as L
    lib, ctx = env
    blocks = log_blocks(lib)
    j = (O.fixture_plain("compression_66k_JSON") * 4)[:65536]
    try:
        for key, v in ((b"compress_depth", 16), (b"compress_subwindows", 4), (b"compress_deterministic", 1), (b"compress_sliding_window", 0)):
            assert lib.lz4flex_set_tuning(ctx, key, v) == 0
        for b in (blocks[5], j, (j * 4)[:200000]):
            out, out_off, out_len, st = run_batch(lib, ctx, [b], L.MEM_DEVICE)
            check_against_model([b], 16, out, out_off, out_len, st)
    finally:
        for key, v in ((b"compress_subwindows", 0), (b"compress_deterministic", 0), (b"compress_sliding_window", 2)):
            assert lib.lz4flex_set_tuning(ctx, key, v) == 0
    got = {}
    for depth in (4, 16):
        assert lib.lz4flex_set_tuning(ctx, b"compress_depth", depth) == 0
        out, out_off, out_len, st = run_batch(lib, ctx, [j], L.MEM_HOST)
        check_against_model([j], depth, out, out_off, out_len, st)
        got[depth] = bytes(out[int(out_off[0]):int(out_off[0]) + int(out_len[0])])
    assert got[4] != got[16]
    assert lib.lz4flex_set_tuning(ctx, b"compress_depth", 16) == 0


def test_every_decoder_reads_high_blocks(env):
    from lz4_flex_amd import block
    lib, ctx = env
    blocks = batch1()
    comp = [model(b, 16) for b in blocks]
    src = np.frombuffer(b"".join(comp), dtype=np.uint8)
    in_len = np.array([len(c) for c in comp], dtype=np.uint32)
    in_off = (np.cumsum(in_len.astype(np.uint64)) - in_len).astype(np.uint64)
    cap = np.array([len(b) for b in blocks], dtype=np.uint32)
    out_off = (np.cumsum(cap.astype(np.uint64)) - cap).astype(np.uint64)
    plain = np.frombuffer(b"".join(blocks), dtype=np.uint8)
    size, st = block.decompressed_size_batch(src, in_off, in_len, ctx=ctx)
    assert not st.any() and size.tolist() == cap.tolist()
    try:
        for variant in (0, 4, 7, 13):
            assert lib.lz4flex_set_tuning(ctx, b"decompress_variant", variant) == 0
            out = np.zeros(plain.size + 1, dtype=np.uint8)
            out_len, st, _ = block.decompress_batch(src, in_off, in_len, out, out_off, cap, ctx=ctx)
            assert not st.any() and out_len.tolist() == cap.tolist(), variant
            assert np.array_equal(out[:-1], plain), variant
    finally:
        assert lib.lz4flex_set_tuning(ctx, b"decompress_variant", 0) == 0


@pytest.fixture
def high_default():
    """this thread's default context (the scalar calls, the frame layer) in mode high; fast again afterwards"""
    from lz4_flex_amd import block
    block.set_compress_mode("high")
    block.set_compress_depth(16)
    yield block
    block.set_compress_mode("fast")
    block.set_compress_depth(16)


def test_scalar_and_packed_entries(high_default):
    from lz4_flex_amd import _lib as L
    block = high_default
    j = O.fixture_plain("compression_66k_JSON")
    table = block.CompressTable.small()
    lib = L.load()
    for data in (j, (j * 4)[:98305], b"", b"abcd" * 5):
        assert block.compress(data) == model(data, 16)
        out = bytearray(4 + block.get_maximum_output_size(len(data)))
        n = lib.lz4flex_compress_prepend_size(data, len(data), (C.c_uint8 * len(out)).from_buffer(out), len(out))
        assert bytes(out[:n]) == len(data).to_bytes(4, "little") + model(data, 16)
        out = bytearray(block.get_maximum_output_size(len(data)))
        n = block.compress_into_with_table(data, out, table)
        assert bytes(out[:n]) == model(data, 16)
    # the packed stream's payloads are the batch's
    blocks = [j[:5000], (j * 2)[100:100 + 70000], b"", j[7:4103]]
    src = np.frombuffer(b"".join(blocks), dtype=np.uint8)
    in_len = np.array([len(b) for b in blocks], dtype=np.uint32)
    in_off = (np.cumsum(in_len.astype(np.uint64)) - in_len).astype(np.uint64)
    out = np.zeros(sum(O.max_out(len(b)) + 4 for b in blocks), dtype=np.uint8)
    for prepend in (True, False):
        out_off, out_len, st = block.compress_batch_packed(src, in_off, in_len, out, prepend_size=prepend)
        assert not st.any()
        for k, b in enumerate(blocks):
            got = bytes(out[int(out_off[k]):int(out_off[k]) + int(out_len[k])])
            assert got == (len(b).to_bytes(4, "little") if prepend else b"") + model(b, 16), (prepend, k)


def test_frames(high_default):
    from lz4_flex_amd import frame
    block = high_default
    data = (O.fixture_plain("compression_66k_JSON") * 4)[:3 * 65536 + 17]
    for sums in (False, True):
        fi = frame.FrameInfo(block_size=frame.BlockSize.Max64KB, block_mode=frame.BlockMode.Independent, block_checksums=sums)
        one = frame.compress_frame(data, fi)
        many = frame.compress_frames([data, data[:70000]], fi)
        assert many[0] == one
        for f, d in ((one, data), (many[1], data[:70000])):
            assert O.frame_decompress(f, len(d))[:2] == (0, d)
            assert O.c_frame_decompress(f, len(d)) == d
        block.set_compress_mode("fast")
        try:
            assert len(one) < len(frame.compress_frame(data, fi))
        finally:
            block.set_compress_mode("high")
        # the blocks are the model's
        body = one[7:]
        for k in range(4):
            raw = data[k * 65536:(k + 1) * 65536]
            m = model(raw, 16)
            want, bit = (m, 0) if len(m) < len(raw) else (raw, 1 << 31)      # (the last 17 bytes are stored raw: frame/compress.rs:301-306)
            assert int.from_bytes(body[:4], "little") == len(want) | bit and body[4:4 + len(want)] == want, k
            body = body[4 + len(want) + (4 if sums else 0):]
    # a Linked frame: compress_mode 0's bytes
    fi = frame.FrameInfo(block_size=frame.BlockSize.Max64KB, block_mode=frame.BlockMode.Linked)
    one, many = frame.compress_frame(data, fi), frame.compress_frames([data, data[:70000]], fi)
    block.set_compress_mode("fast")
    try:
        assert one == frame.compress_frame(data, fi) and many == frame.compress_frames([data, data[:70000]], fi)
    finally:
        block.set_compress_mode("high")
    assert O.frame_decompress(one, len(data))[:2] == (0, data)


def test_dictionary_entries_give_mode_0_bytes(high_default):
    block = high_default
    j = O.fixture_plain("compression_66k_JSON")
    blocks = [j[1000:41000], j[20000:20100], (j * 2)[5:70005]]      # (32 KiB and more lie in front of the second and the third)
    src = np.frombuffer(b"".join(blocks), dtype=np.uint8)
    in_len = np.array([len(b) for b in blocks], dtype=np.uint32)
    in_off = (np.cumsum(in_len.astype(np.uint64)) - in_len).astype(np.uint64)
    cap = np.array([O.max_out(len(b)) for b in blocks], dtype=np.uint32)
    out_off = (np.cumsum(cap.astype(np.uint64)) - cap).astype(np.uint64)
    # (the fixture has 66 675 bytes: the second dictionary's 40 000 come from two copies of it -- j[30000:70000] was 36 675 bytes, and
    # the 40 000 of d_len reached 3 325 bytes past the buffer, into whatever lay behind it: bytes that changed from call to call)
    dicts = np.frombuffer(j[:4096] + (j * 2)[30000:30000 + 40000], dtype=np.uint8)
    d_off, d_len = np.array([0, 4096, 0], dtype=np.uint64), np.array([4096, 40000, 0], dtype=np.uint32)
    assert len(dicts) == int(d_off[1] + d_len[1])

    def every_entry():
        res = []
        with block.DictSet([dicts[:4096], dicts[4096:]]) as ds:
            for call in (lambda o: block.compress_batch_with_dict(src, in_off, in_len, dicts, d_off, d_len, o, out_off, cap),
                         lambda o: block.compress_batch_with_shared_dict(src, in_off, in_len, dicts[:4096], o, out_off, cap),
                         lambda o: block.compress_batch_with_dict_set(src, in_off, in_len, [0, 1, 0xFFFFFFFF], ds, o, out_off, cap)):
                out = np.zeros(int(cap.sum()), dtype=np.uint8)
                out_len, st = call(out)
                assert not st.any()
                res.append([bytes(out[int(o):int(o) + int(n)]) for o, n in zip(out_off, out_len)])
        return res

    high = every_entry()
    block.set_compress_mode("fast")
    try:
        fast = every_entry()
    finally:
        block.set_compress_mode("high")
    assert high == fast
    # a raw batch with history flags: the flags are not read, the blocks are independent ones
    out = np.zeros(int(cap.sum()), dtype=np.uint8)
    out_len, st = block.compress_batch(src, in_off, in_len, out, out_off, cap, flags=[0, 32768 << 8, 32768 << 8])
    assert not st.any()
    for k, b in enumerate(blocks):
        assert bytes(out[int(out_off[k]):int(out_off[k]) + int(out_len[k])]) == model(b, 16), k
