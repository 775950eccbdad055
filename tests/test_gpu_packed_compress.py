"""GPU tests of lz4flex_compress_batch_packed (the encoders + lz4_packed.hip): under compress_mode exact the packed stream is the
concatenation of the oracle's size-prepended encodings at out_off; in fast mode the payloads are lz4flex_compress_batch's; the fit rule
on the output and on the scratch slots; compress -> decompress on the device with nothing computed on the host in between."""
import ctypes as C
import random

import numpy as np
import pytest

import oracle_api as O
import packed_cases as P

pytestmark = pytest.mark.gpu

MEMS = ["device", "host"]


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


@pytest.fixture(scope="module")
def inputs():
    """300 blocks of 0 ... 70 000 bytes (JSON, text, zeros, random bytes) and one of 300 000; with the oracle's encodings"""
    rnd = random.Random(77)
    json, text = O.fixture_plain("compression_66k_JSON"), O.fixture_plain("compression_65k")
    noise = bytes(rnd.getrandbits(8) for _ in range(70000))
    lens = [0, 1, 4, 5, 12, 13, 14, 70000, 65536, 65535, 65534] + [rnd.randint(0, 70000) if k % 3 else rnd.randint(0, 300) for k in range(289)]
    plains = []
    for k, ln in enumerate(lens):
        src = (json, text, bytes(70000), noise)[k % 4]
        a = rnd.randint(0, max(0, len(src) - ln))
        plains.append((src * 2)[a:a + ln])
    assert len(plains) == 300
    plains.insert(150, (json * 5)[:300000])
    return plains, [O.compress(p) for p in plains]


def check_stream(got, want_blocks, align, total_cap, what, lost_scratch=()):
    """want_blocks[i]: the bytes block i must have in the stream.  The layout is the cumsum of the lengths of the blocks the encoder
    produced (a block without a scratch slot takes no room); the fit rule; canaries everywhere else"""
    n = len(want_blocks)
    sizes = np.array([0 if i in lost_scratch else len(b) for i, b in enumerate(want_blocks)], np.uint64)
    off = P.layout(sizes, align)
    assert (got["out_off"] == off).all(), (what, np.nonzero(got["out_off"] != off)[0][:4])
    fits = off[:n] + sizes <= np.uint64(total_cap)
    ok = fits & np.array([i not in lost_scratch for i in range(n)])
    want_st = np.where(ok, 0, P.E_OUTPUT_TOO_SMALL).astype(np.int32)
    assert (got["status"] == want_st).all(), (what, np.nonzero(got["status"] != want_st)[0][:4])
    assert (got["out_len"] == np.where(ok, sizes, 0)).all(), what
    image = np.full(got["out"].size, P.CANARY, np.uint8)
    for i in np.nonzero(ok)[0]:
        image[int(off[i]):int(off[i]) + len(want_blocks[i])] = np.frombuffer(want_blocks[i], np.uint8)
    bad = np.nonzero(got["out"] != image)[0]
    assert bad.size == 0, "%s: %d bytes of the stream differ, first at %d" % (what, bad.size, bad[0])
    return off, ok


@pytest.mark.parametrize("align", [1, 16])
@pytest.mark.parametrize("mem", MEMS)
def test_exact_mode_is_the_reference_stream(lib, ctx, inputs, mem, align):
    plains, comps = inputs
    assert lib.lz4flex_set_tuning(ctx, b"compress_mode", 1) == 0
    buf, offs, lens = P.pack(plains)
    for prepend in (1, 0):
        want = [(P.le32(len(p)) if prepend else b"") + c for p, c in zip(plains, comps)]
        room = int(P.layout([len(w) for w in want], align)[-1])
        got = P.compress(lib, ctx, buf, offs, lens, prepend, align, room, room, mem, big=True)
        check_stream(got, want, align, room, "exact %s align=%d prepend=%d" % (mem, align, prepend))


@pytest.mark.parametrize("mem", MEMS)
def test_fast_mode_payloads_are_compress_batch(lib, ctx, inputs, mem):
    from lz4_flex_amd import block
    plains, _comps = inputs
    buf, offs, lens = P.pack(plains)
    n = len(plains)
    caps = np.array([O.max_out(len(p)) for p in plains], np.uint32)
    slot_off = P.layout(caps, 1)
    plain_out = np.zeros(int(slot_off[-1]) + 64, np.uint8)
    out_len, status = block.compress_batch(buf, offs, lens, plain_out, slot_off[:-1], caps, ctx=ctx)
    assert (status == 0).all()
    payloads = [plain_out[int(slot_off[i]):int(slot_off[i]) + int(out_len[i])].tobytes() for i in range(n)]
    for p, c in zip(plains, payloads):
        assert O.decompress(c, len(p)) == ("ok", p)
    want = [P.le32(len(p)) + c for p, c in zip(plains, payloads)]
    room = int(P.layout([len(w) for w in want], 16)[-1])
    got = P.compress(lib, ctx, buf, offs, lens, 1, 16, room, room, mem, big=True)
    check_stream(got, want, 16, room, "fast " + mem)


@pytest.mark.parametrize("mem", MEMS)
def test_total_cap_in_the_middle(lib, ctx, inputs, mem):
    plains, comps = inputs
    assert lib.lz4flex_set_tuning(ctx, b"compress_mode", 1) == 0
    buf, offs, lens = P.pack(plains)
    want = [P.le32(len(p)) + c for p, c in zip(plains, comps)]
    off = P.layout([len(w) for w in want], 16)
    for total_cap in (int(off[len(want) // 2]), int(off[-2]) + len(want[-1]) - 1):      # in the middle; one byte short of the last block
        got = P.compress(lib, ctx, buf, offs, lens, 1, 16, total_cap, int(off[-1]), mem, big=True)
        _off, ok = check_stream(got, want, 16, total_cap, "cap %s %d" % (mem, total_cap))
        assert (got["out"][total_cap:] == P.CANARY).all() and 0 < ok.sum() < len(want)


def test_scratch_too_small_on_the_device(lib, ctx, inputs):
    """a DEVICE call cannot see the lengths: the blocks whose scratch slot ends behind scratch_cap are flagged, the others are intact"""
    from lz4_flex_amd import _lib
    plains, comps = inputs
    assert lib.lz4flex_set_tuning(ctx, b"compress_mode", 1) == 0
    buf, offs, lens = P.pack(plains)
    want = [P.le32(len(p)) + c for p, c in zip(plains, comps)]
    slots = P.layout([O.max_out(len(p)) + 4 for p in plains], 1)
    k = 200
    scratch_cap = int(slots[k]) + 3                  # block k's slot starts inside and ends outside
    lost = {i for i in range(len(plains)) if int(slots[i + 1]) > scratch_cap}
    assert min(lost) == k and len(lost) > 50
    room = int(P.layout([len(w) for w in want], 1)[-1])
    got = P.compress(lib, ctx, buf, offs, lens, 1, 1, room, room, "device", big=True, scratch_cap=scratch_cap)
    check_stream(got, want, 1, room, "scratch", lost_scratch=lost)
    # a HOST call sees them: refused as a whole, exactly below the sum of the slots
    p = lambda a: C.c_void_p(a.ctypes.data)
    res = [np.zeros(len(plains) + 1, np.uint64), np.zeros(len(plains), np.uint32), np.zeros(len(plains), np.int32)]
    out = np.zeros(room, np.uint8)
    call = lambda cap: lib.lz4flex_compress_batch_packed(ctx, p(buf), p(offs), p(lens), len(plains), 1, None, cap, p(out), room, 1, p(res[0]), p(res[1]),
                                                         p(res[2]), None, _lib.MEM_HOST, None)
    assert call(int(slots[-1]) - 1) == -_lib.E_INVALID_ARG and call(int(slots[-1])) == 0
    assert (res[2] == 0).all() and int(res[0][-1]) == room


def test_round_trip_on_the_device(inputs):
    """compress_blocks_packed_device -> decompress_blocks_packed_device: the second call's in_off / in_len are the first one's device
    tensors; the host computes nothing in between"""
    import torch
    from lz4_flex_amd import block
    plains, _comps = inputs
    buf, offs, lens = P.pack(plains)
    src = P._dev(buf)
    n = len(plains)
    comp, c_off, c_len, c_st = block.compress_blocks_packed_device(src, P._dev(offs), P._dev(lens), buf.size + 1024 * n, big_blocks=True)
    out, out_off, out_len, status = block.decompress_blocks_packed_device(comp, c_off[:n], c_len, buf.size + 16 * n, align=16, big_blocks=True)
    torch.cuda.synchronize()
    assert int(c_st.abs().sum()) == 0 and int(status.abs().sum()) == 0
    assert (out_len.cpu().numpy().view(np.uint32) == lens).all()
    assert (out_off.cpu().numpy().view(np.uint64) == P.layout(lens, 16)).all()
    host = out.cpu().numpy()
    for p, o in zip(plains, out_off.tolist()):
        assert host[o:o + len(p)].tobytes() == p
    # host buffers: the same stream
    h_comp = np.zeros(buf.size + 1024 * n, np.uint8)
    h_off, h_len, h_st = block.compress_batch_packed(buf, offs, lens, h_comp)
    assert (h_st == 0).all() and (h_off.view(np.int64) == c_off.cpu().numpy()).all() and (h_len.view(np.int32) == c_len.cpu().numpy()).all()
    assert (h_comp[:int(h_off[-1])] == comp[:int(h_off[-1])].cpu().numpy()).all()


@pytest.mark.parametrize("mem", MEMS)
def test_tiny_batches_around_the_scan_tile(lib, ctx, mem):
    T = lib.lz4flex_get_tuning(None, b"packed_scan_tile")
    ns = [1, 2, T - 1, T, T + 1, 3 * T + 7]
    if 256 * T + T + 1 <= 2 * 1024 * 1024:         # (beyond the first-level reach of the one workgroup that scans the tile sums)
        ns.append(256 * T + T + 1)
    for n in ns:
        lens = ((np.arange(n, dtype=np.int64) * 5 + np.arange(n, dtype=np.int64) // 3) % 8 + 1).astype(np.uint32)       # 1 ... 8 bytes
        offs = np.zeros(n, np.uint64)
        np.cumsum(lens[:-1], dtype=np.uint64, out=offs[1:])
        buf = ((np.arange(int(lens.sum()) + 8) * 131) >> 3).astype(np.uint8)
        for align in (1, 16):
            # inputs below 13 bytes are one run of literals: token, the bytes (compress.rs:343-346); behind the LE u32 length
            sizes = lens.astype(np.uint64) + np.uint64(5)
            room = int(P.layout(sizes, align)[-1])
            got = P.compress(lib, ctx, buf, offs, lens, 1, align, room, room, mem)
            off = P.layout(got["out_len"], align)
            assert (got["status"] == 0).all() and (got["out_len"] == sizes).all(), (n, align)
            assert (got["out_off"] == off).all(), (n, align, np.nonzero(got["out_off"] != off)[0][:4])
            o = off[:n].astype(np.int64)
            image = np.full(got["out"].size, P.CANARY, np.uint8)
            image[o] = lens
            image[o + 1] = image[o + 2] = image[o + 3] = 0
            image[o + 4] = lens << 4
            for k in range(8):
                sel = lens > k
                image[o[sel] + 5 + k] = buf[offs[sel].astype(np.int64) + k]
            bad = np.nonzero(got["out"] != image)[0]
            assert bad.size == 0, (n, align, bad[:4])
