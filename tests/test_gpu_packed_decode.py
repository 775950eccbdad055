"""GPU tests of lz4flex_decompress_batch_packed (lz4_packed.hip + the decoders): the layout is numpy's uint64 cumsum of the sizes rounded
up to `align`, every block gets what the oracle's decompress_into gives it in a sink of its slot's size, canaries sit behind off[n], in
every alignment gap and behind every short block; MEM_DEVICE and MEM_HOST, align 1 / 16 / 256, all three size modes, the fit rule,
offsets beyond 4 GiB, pinned decoders."""
import ctypes as C
import random

import numpy as np
import pytest

import corpus
import oracle_api as O
import packed_cases as P

pytestmark = pytest.mark.gpu

PREPENDED, GIVEN, SCAN = 0, 1, 2
MEMS = ["device", "host"]
ALIGNS = [1, 16, 256]


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


# ---- scan boundaries, on tiny blocks ---------------------------------------------------------------------------------------------
TINY = [(b"\x00", b""), (b"\x10a", b"a"), (b"\x20ab", b"ab")]          # one to three bytes that decode to 0, 1 or 2


def tiny_batch(n, prepend):
    """n tiny blocks, mixed, as one buffer: (buf, off, len, kind)"""
    kind = (np.arange(n, dtype=np.int64) * 7 + np.arange(n, dtype=np.int64) // 5) % 3
    raw_len = kind + 1
    head = 4 if prepend else 0
    lens = (raw_len + head).astype(np.uint32)
    offs = np.zeros(n, np.uint64)
    np.cumsum(lens[:-1], dtype=np.uint64, out=offs[1:])
    buf = np.zeros(int(lens.sum()) + 8, np.uint8)
    o = offs.astype(np.int64)
    if prepend:
        buf[o] = kind                                                   # the LE u32 prefix: the decoded size (0, 1, 2)
    buf[o + head] = kind << 4                                           # the token: `kind` literals, the end of the block
    buf[(o + head + 1)[kind >= 1]] = ord("a")
    buf[(o + head + 2)[kind >= 2]] = ord("b")
    return buf, offs, lens, kind


def check_tiny(got, kind, align, what):
    n = len(kind)
    sizes = kind.astype(np.uint64)
    off = P.layout(sizes, align)
    assert (got["out_off"] == off).all(), (what, np.nonzero(got["out_off"] != off)[0][:4])
    assert (got["out_cap"] == sizes).all() and (got["out_len"] == sizes).all(), what
    assert (got["status"] == 0).all() and (got["detail"] == 0).all(), (what, got["status"][got["status"] != 0][:4])
    image = np.full(got["out"].size, P.CANARY, np.uint8)
    o = off[:n].astype(np.int64)
    image[o[kind >= 1]] = ord("a")
    image[o[kind >= 2] + 1] = ord("b")
    bad = np.nonzero(got["out"] != image)[0]
    assert bad.size == 0, "%s: %d output bytes differ, first at %d" % (what, bad.size, bad[0])


def test_tiny_blocks_are_what_the_oracle_says():
    for comp, plain in TINY:
        assert O.decompress(comp, len(plain)) == ("ok", plain)


def scan_sizes(lib):
    T = lib.lz4flex_get_tuning(None, b"packed_scan_tile")
    assert T >= 64
    # the one workgroup that scans the tile sums has 256 threads: up to 256 tiles a thread takes one sum, beyond it several -- the
    # second level's first-level reach is 256 T blocks (262 144 for T = 1 024: below the 2 M blocks at which this case would be skipped)
    ns = [1, 2, T - 1, T, T + 1, 3 * T + 7]
    if 256 * T + T + 1 <= 2 * 1024 * 1024:
        ns.append(256 * T + T + 1)
    return ns


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("mem", MEMS)
def test_scan_boundaries(lib, ctx, mem, align):
    for n in scan_sizes(lib):
        buf, offs, lens, kind = tiny_batch(n, True)
        total = int(P.layout(kind, align)[-1])
        got = P.decode(lib, ctx, buf, offs, lens, PREPENDED, None, align, total, total, mem)
        check_tiny(got, kind, align, "n=%d %s align=%d" % (n, mem, align))


@pytest.mark.parametrize("mem", MEMS)
def test_scan_boundaries_given_and_scan_modes(lib, ctx, mem):
    ns = scan_sizes(lib)
    for n in (ns[4], ns[5]):
        buf, offs, lens, kind = tiny_batch(n, False)
        total = int(P.layout(kind, 16)[-1])
        for mode in (GIVEN, SCAN):
            got = P.decode(lib, ctx, buf, offs, lens, mode, kind.astype(np.uint32) if mode == GIVEN else None, 16, total, total, mem)
            check_tiny(got, kind, 16, "n=%d %s mode=%d" % (n, mem, mode))


# ---- the three size modes on real blocks -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch():
    """[(raw block, size of its slot)]: the reference's decoder KATs with their capacities, its size-prepended no-panic inputs with
    their own prefixes, ~200 oracle-compressed blocks of 0 ... 70 000 bytes with their true sizes, one prefix above and one below the
    true size; and what the oracle's decompress_into gives each in a sink of that size"""
    rnd = random.Random(2024)
    items = [(c, cap) for c, cap, d, _want in corpus.DECODER_KATS if d is None]
    items += [(c[4:], int.from_bytes(c[:4], "little")) for c in corpus.NO_PANIC_SIZE_PREPENDED]
    json, text = O.fixture_plain("compression_66k_JSON"), O.fixture_plain("compression_65k")
    noise = bytes(rnd.getrandbits(8) for _ in range(70000))
    lens = [0, 1, 4, 12, 13, 70000, 65536, 65535] + [rnd.randint(0, 70000) if k % 3 else rnd.randint(0, 600) for k in range(192)]
    for k, ln in enumerate(lens):
        src = (json, text, bytes(70000), noise)[k % 4]
        a = rnd.randint(0, max(0, len(src) - ln))
        plain = (src * 2)[a:a + ln]
        items.append((O.compress(plain), len(plain)))
    big = O.compress(json[:30000])
    items.insert(40, (big, 30000 + 100))          # a prefix larger than the true size: out_len below the slot
    items.insert(90, (big, 30000 - 7))            # a prefix smaller than it: OutputTooSmall {expected, actual = prefix}
    results = [P.oracle_block(c, s) for c, s in items]
    assert results[40][:2] == (0, 30000) and results[90][0] == P.E_OUTPUT_TOO_SMALL and results[90][2][1] == 30000 - 7
    assert {r[0] for r in results} >= {0, 1, 2, 3, 4, 5}
    return items, results


SHORT_AT = 17        # PREPENDED batches: where the block of in_len 3 goes


def prepended_inputs(items, results):
    blocks = [P.le32(s) + c for c, s in items]
    sizes = [s for _c, s in items]
    res = list(results)
    pre = [0] * len(items)
    blocks.insert(SHORT_AT, b"\x09\x00\x00")
    sizes.insert(SHORT_AT, 0)
    res.insert(SHORT_AT, None)
    pre.insert(SHORT_AT, P.E_EXPECTED_ANOTHER_BYTE)
    return blocks, np.array(sizes, np.uint64), res, pre


def scan_inputs(items):
    """raw blocks without sizes: the slot is what decompress_into produces in an unbounded sink, or empty with the block's error"""
    sizes, res, pre = [], [], []
    for c, _s in items:
        st, ln, _det, data = P.oracle_block(c, 255 * len(c) + 64)
        sizes.append(ln)
        pre.append(st)
        res.append((0, ln, (0, 0), data) if st == 0 else None)
    return np.array(sizes, np.uint64), res, pre


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("mem", MEMS)
def test_prepended(lib, ctx, batch, mem, align):
    blocks, sizes, res, pre = prepended_inputs(*batch)
    buf, offs, lens = P.pack(blocks, odd=True)
    total = int(P.layout(sizes, align)[-1])
    got = P.decode(lib, ctx, buf, offs, lens, PREPENDED, None, align, total, total, mem)
    want = P.expect_decode(res, sizes, pre, align, total)
    P.check_decode(got, want, "prepended %s align=%d" % (mem, align))
    assert got["status"][SHORT_AT] == P.E_EXPECTED_ANOTHER_BYTE and got["out_cap"][SHORT_AT] == 0 and got["out_off"][SHORT_AT + 1] == got["out_off"][SHORT_AT]
    k = 40 + 1                                     # (behind the short block)
    assert got["out_len"][k] == 30000 and got["out_cap"][k] == 30100
    k = 90 + 1
    assert got["status"][k] == P.E_OUTPUT_TOO_SMALL and got["detail"][k][1] == 30000 - 7 and got["detail"][k][0] > 30000 - 7


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("mem", MEMS)
def test_given_equals_decompress_batch(lib, ctx, batch, mem, align):
    from lz4_flex_amd import block
    items, results = batch
    sizes = np.array([s for _c, s in items], np.uint64)
    buf, offs, lens = P.pack([c for c, _s in items])
    total = int(P.layout(sizes, align)[-1])
    got = P.decode(lib, ctx, buf, offs, lens, GIVEN, sizes.astype(np.uint32), align, total, total, mem)
    P.check_decode(got, P.expect_decode(results, sizes, [0] * len(items), align, total), "given %s align=%d" % (mem, align))
    # lz4flex_decompress_batch on the same slots
    out = np.full(total + P.TAIL, P.CANARY, np.uint8)
    out_len, status, detail = block.decompress_batch(buf, offs, lens, out, got["out_off"][:-1], sizes.astype(np.uint32), ctx=ctx)
    assert (out_len == got["out_len"]).all() and (status == got["status"]).all()
    small = status == P.E_OUTPUT_TOO_SMALL          # (lz4flex_decompress_batch fills the detail of these blocks only)
    assert small.sum() >= 3 and (detail[small] == got["detail"][small]).all()
    for i in np.nonzero(status == 0)[0]:
        o = int(got["out_off"][i])
        assert (out[o:o + int(out_len[i])] == got["out"][o:o + int(out_len[i])]).all(), i


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("mem", MEMS)
def test_scan(lib, ctx, batch, mem, align):
    items, _results = batch
    sizes, res, pre = scan_inputs(items)
    buf, offs, lens = P.pack([c for c, _s in items])
    total = int(P.layout(sizes, align)[-1])
    got = P.decode(lib, ctx, buf, offs, lens, SCAN, None, align, total, total, mem)
    P.check_decode(got, P.expect_decode(res, sizes, pre, align, total), "scan %s align=%d" % (mem, align))
    assert sum(1 for p in pre if p) > 10


def test_scan_equals_decompress_blocks_device(lib, ctx, batch):
    import torch
    from lz4_flex_amd import block
    items, _results = batch
    buf, offs, lens = P.pack([c for c, _s in items])
    sizes, _res, _pre = scan_inputs(items)
    total = int(sizes.sum())
    got = P.decode(lib, ctx, buf, offs, lens, SCAN, None, 1, total, total, "device")
    out, out_off, out_len, status = block.decompress_blocks_device(P._dev(buf), P._dev(offs), P._dev(lens))
    torch.cuda.synchronize()
    assert out.numel() == total == int(got["out_off"][-1])
    assert (out_off.cpu().numpy().view(np.uint64) == got["out_off"][:-1]).all()
    assert (out_len.cpu().numpy().view(np.uint32) == got["out_len"]).all() and (status.cpu().numpy() == got["status"]).all()
    assert (out.cpu().numpy() == got["out"][:total]).all()


# ---- the fit rule ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", MEMS)
def test_fit_rule(lib, ctx, batch, mem):
    blocks, sizes, res, pre = prepended_inputs(*batch)
    buf, offs, lens = P.pack(blocks, odd=True)
    align = 16
    off = P.layout(sizes, align)
    n = len(blocks)
    for total_cap in (int(off[n // 2]), int(off[n]) - 1):
        got = P.decode(lib, ctx, buf, offs, lens, PREPENDED, None, align, total_cap, int(off[n]), mem)
        want = P.expect_decode(res, sizes, pre, align, total_cap)
        P.check_decode(got, want, "fit %s total_cap=%d" % (mem, total_cap))
        assert got["out_off"][n] == off[n]                              # the capacity the batch needs, whatever it was given
        assert (got["out"][total_cap:] == P.CANARY).all()
        lost = np.nonzero(off[:n] + sizes > np.uint64(total_cap))[0]
        assert lost.size >= 1 and (got["status"][lost] == P.E_OUTPUT_TOO_SMALL).all() and (got["out_cap"][lost] == 0).all()
        assert (got["detail"][lost, 0] == (off[:n] + sizes)[lost]).all() and (got["detail"][lost, 1] == total_cap).all()
        kept = np.setdiff1d(np.arange(n), lost)
        assert (got["status"][kept] == want["status"][kept]).all() and (got["status"][kept] == 0).sum() > (50 if total_cap < off[n] - 1 else 150)


@pytest.mark.parametrize("mem", MEMS)
def test_offsets_beyond_4_gib_without_the_memory(lib, ctx, mem):
    real = [b"hello packed world " * 40, b"", bytes(5000)]
    blocks = [P.le32(len(p)) + O.compress(p) for p in real] + [P.le32(0xFFFFFFF0) + O.compress(b"hostile prefix")] * 8
    sizes = np.array([len(p) for p in real] + [0xFFFFFFF0] * 8, np.uint64)
    buf, offs, lens = P.pack(blocks, odd=True)
    for align in (1, 256):
        off = P.layout(sizes, align)
        assert int(off[-1]) > 1 << 34
        total_cap = int(off[3]) + 4096
        got = P.decode(lib, ctx, buf, offs, lens, PREPENDED, None, align, total_cap, total_cap, mem)
        res = [(0, len(p), (0, 0), p) for p in real] + [None] * 8
        P.check_decode(got, P.expect_decode(res, sizes, [0] * 11, align, total_cap), "4 GiB %s align=%d" % (mem, align))
        assert (got["out_off"] == off).all() and (got["status"][:3] == 0).all() and (got["status"][3:] == P.E_OUTPUT_TOO_SMALL).all()


# ---- the layout does not depend on the decoder -----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [13, 7])
def test_pinned_decoders(lib, ctx, batch, variant):
    assert lib.lz4flex_set_tuning(ctx, b"decompress_variant", variant) == 0
    blocks, sizes, res, pre = prepended_inputs(*batch)
    buf, offs, lens = P.pack(blocks, odd=True)
    total = int(P.layout(sizes, 16)[-1])
    got = P.decode(lib, ctx, buf, offs, lens, PREPENDED, None, 16, total, total, "device")
    P.check_decode(got, P.expect_decode(res, sizes, pre, 16, total), "variant %d" % variant)


def test_torch_wrappers_do_not_need_the_sizes():
    import torch
    from lz4_flex_amd import block
    dev = torch.device("cuda", 0)
    plains = [b"abc" * 1000, b"", bytes(range(256)) * 9, b"x"]
    blocks = [P.le32(len(p)) + O.compress(p) for p in plains]
    buf, offs, lens = P.pack(blocks, odd=True)
    out, out_off, out_len, status = block.decompress_blocks_packed_device(P._dev(buf), P._dev(offs), P._dev(lens), 1 << 16, align=16)
    torch.cuda.synchronize()
    assert out.numel() == 1 << 16 and out_off.numel() == 5 and status.device == dev and int(status.abs().sum()) == 0
    for p, o, ln in zip(plains, out_off.tolist(), out_len.tolist()):
        assert o % 16 == 0 and out[o:o + ln].cpu().numpy().tobytes() == p
    # host buffers
    host = np.full(1 << 16, P.CANARY, np.uint8)
    h_off, h_cap, h_len, h_st, _det = block.decompress_batch_packed(buf, offs, lens, host, align=16)
    assert (h_off.view(np.int64) == out_off.cpu().numpy()).all() and (h_st == 0).all() and (h_cap == [len(p) for p in plains]).all()
    for p, o, ln in zip(plains, h_off.tolist(), h_len.tolist()):
        assert host[o:o + ln].tobytes() == p
