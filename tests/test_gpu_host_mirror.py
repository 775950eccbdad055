"""GPU (-m gpu): a MEM_HOST call of the C ABI mirrors the caller's host layout on the device (lz4_host_stage.h, capi.cpp) and runs what a
MEM_DEVICE call runs -- so the same bytes through both give the same return code, the same result arrays and the same bytes in every good
block, and in the host buffer nothing outside a good block's [out_off, out_off + out_len) is written.

The layouts are the smallest at which staging can go wrong: the span starts at byte 4 099 of the buffer, the blocks lie in shuffled
order with gaps of 1 ... 37 bytes in the input and in the output buffer, one block has length 0, one is made to fail.  Block counts: 5
(the small path: one image each way), 9 (the general path, a copy per block), 24 with outputs that tile their span, the last one short
(one copy of the span), 24 with a failure (the pack kernel), and one block of 70 000 bytes (what the lengths say about large blocks;
the device call says LZ4FLEX_MEM_BIG_BLOCKS).  The compress entries run "compress_mode" 1: the oracle's bytes, decoded by the oracle."""
import ctypes as C

import numpy as np
import pytest

import dict_cases as D
import oracle_api as O
from test_gpu_capi_batch import Arrays, _ctx

pytestmark = pytest.mark.gpu

START = 4099
KINDS = ["json", "text", "log", "random"]


@pytest.fixture(scope="module")
def env():
    import torch
    from lz4_flex_amd import _lib
    lib = _lib.load()
    assert lib.lz4flex_device_count() >= 1, _lib.last_error()
    return lib, _lib, torch


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def lengths(n, rng, top=700):
    """n block lengths in 0 ... top: one 0, one `top`"""
    lens = [int(v) for v in rng.integers(1, top + 1, n)]
    lens[0], lens[min(2, n - 1)] = top, 0
    return lens


def scattered(rng, sizes):
    """offsets for blocks of `sizes` bytes laid from byte START on in shuffled order, 1 ... 37 bytes between them; the bytes they need"""
    off, pos = [0] * len(sizes), START
    for i in rng.permutation(len(sizes)):
        off[i] = pos
        pos += sizes[i] + int(rng.integers(1, 38))
    return off, pos + 64


def tiled(sizes):
    off, pos = [], START
    for s in sizes:
        off.append(pos)
        pos += s
    return off, pos + 64


def buffer_of(rng, nbytes, off=(), parts=()):
    """`nbytes` of noise with `parts` at `off`"""
    buf = rng.integers(0, 256, nbytes, dtype=np.uint8)
    for o, p in zip(off, parts):
        buf[o:o + len(p)] = u8(p)
    return buf


def both(env, arrays, call, big=False):
    """the call on the arrays in host memory and on their copies in device memory: (rc, arrays) of each"""
    lib, L, torch = env
    res = []
    for device in (False, True):
        a = Arrays(torch, device, **{k: v.copy() for k, v in arrays.items()})
        mem = (L.MEM_DEVICE | (L.MEM_BIG_BLOCKS if big else 0)) if device else L.MEM_HOST
        rc = call(a.ptr, mem)
        res.append((rc, a.fetch()))
    return res


def same_results(res, arrays, results, sink="sink", off="out_off", length="out_len", status="status", pos=None):
    """equal return code and result arrays; equal bytes in every good block; the host buffer untouched everywhere else.  The good blocks'
    (offset, length) pairs, for the caller's own look at the bytes.  "detail": the rows the header defines, those of the blocks that
    answered OutputTooSmall (a decoder may leave the other rows as it found them, and a MEM_HOST call finds the arena's)."""
    (rc_h, h), (rc_d, d) = res
    assert rc_h == rc_d == 0, (rc_h, rc_d)
    for name in results:
        if name == "detail":
            small = np.repeat(h[status] == 1, 2)
            assert np.array_equal(h[name][small], d[name][small]), (name, h[name], d[name])
            continue
        assert np.array_equal(h[name], d[name]), (name, h[name], d[name])
    untouched = np.ones(len(arrays[sink]), bool)
    good = []
    for i in range(len(arrays["in_len"])):
        if status is not None and h[status][i] != 0:
            good.append(None)
            continue
        o = int(h[off][i]) + (int(arrays[pos][i]) if pos else 0)
        m = int(h[length][i])
        assert np.array_equal(h[sink][o:o + m], d[sink][o:o + m]), i
        untouched[o:o + m] = False
        good.append((o, m))
    assert np.array_equal(h[sink][untouched], arrays[sink][untouched]), "a MEM_HOST call wrote outside its good blocks"
    return h, good


# ------------------------------------------------------------------------------------------------ the batch of the plain codec entries
SHAPES = ["n5", "n9", "n24-tiled", "n24-fail", "big"]


def decode_job(shape, seed, dicts=None, prefix=None):
    """compressed blocks scattered in `src`, sinks scattered (tiled: back to back) in `sink`; block `fail`'s sink is one byte short"""
    rng = np.random.default_rng(seed)
    n = {"n5": 5, "n9": 9, "n24-tiled": 24, "n24-fail": 24, "big": 1}[shape]
    lens = [70000] if shape == "big" else lengths(n, rng)
    # (n24-fail: blocks that do not shrink -- the packed results have to fit the input region for the pack kernel to take them)
    kinds = ["random"] * n if shape == "n24-fail" else [KINDS[i % 4] for i in range(n)]
    plains = [D.block(k, m, seed + i) for i, (k, m) in enumerate(zip(kinds, lens))]
    pre = [D.block("text", int(rng.integers(1, 300)), 50 + i) for i in range(n)] if prefix else [b""] * n
    comps = [O.compress_with_dict(p, dicts[i]) if dicts else O.compress_with_dict(p, pre[i]) if prefix else O.compress(p) for i, p in enumerate(plains)]
    fail = None if shape in ("n24-tiled", "big") else n - 2
    caps = [len(q) + m + 5 for q, m in zip(pre, lens)]
    if shape == "n24-tiled":
        caps = lens[:-1] + [lens[-1] + 9]
    if fail is not None:
        caps[fail] = len(pre[fail]) + lens[fail] - 1
    in_off, in_bytes = scattered(rng, [len(c) for c in comps])
    out_off, out_bytes = tiled(caps) if shape == "n24-tiled" else scattered(rng, caps)
    arrays = dict(src=buffer_of(rng, in_bytes, in_off, comps), in_off=np.array(in_off, np.uint64), in_len=np.array([len(c) for c in comps], np.uint32),
                  sink=buffer_of(rng, out_bytes, out_off, pre), out_off=np.array(out_off, np.uint64), cap=np.array(caps, np.uint32),
                  out_len=np.full(n, 0xDEADBEEF, np.uint32), status=np.full(n, -1, np.int32), detail=np.full(2 * n, 0xEE, np.uint64),
                  pos=np.array([len(q) for q in pre], np.uint32))
    return arrays, plains, fail


def check_decoded(h, good, plains, fail):
    for i, g in enumerate(good):
        assert (g is None) == (i == fail), (i, h["status"])
        if g:
            assert h["sink"][g[0]:g[0] + g[1]].tobytes() == plains[i], i


@pytest.mark.parametrize("shape", SHAPES)
def test_decompress_batch(env, shape):
    lib, L, torch = env
    arrays, plains, fail = decode_job(shape, 11)
    ctx = _ctx(lib)
    try:
        def call(p, mem):
            return lib.lz4flex_decompress_batch(ctx, p("src"), p("in_off"), p("in_len"), len(plains), p("sink"), p("out_off"), p("cap"), p("out_len"),
                                                p("status"), p("detail"), mem, None)
        h, good = same_results(both(env, arrays, call, big=shape == "big"), arrays, ["out_len", "status", "detail"])
        check_decoded(h, good, plains, fail)
    finally:
        lib.lz4flex_ctx_destroy(ctx)


@pytest.mark.parametrize("mode", ["dicts", "prefixes"])
def test_decompress_batch_ex(env, mode):
    lib, L, torch = env
    rng = np.random.default_rng(5)
    n = 9
    dicts = [D.block(KINDS[i % 3], int(rng.integers(1, 500)), 80 + i) for i in range(n)] if mode == "dicts" else None
    arrays, plains, fail = decode_job("n9", 23, dicts=dicts, prefix=mode == "prefixes")
    if dicts:
        d_off, d_bytes = scattered(rng, [len(d) for d in dicts])
        arrays.update(dic=buffer_of(rng, d_bytes, d_off, dicts), dict_off=np.array(d_off, np.uint64), dict_len=np.array([len(d) for d in dicts], np.uint32))
    ctx = _ctx(lib)
    try:
        def call(p, mem):
            ext = L.DecompressExt(p("dic"), p("dict_off"), p("dict_len"), None, None, 0) if dicts else L.DecompressExt(None, None, None, p("pos"), None, 0)
            return lib.lz4flex_decompress_batch_ex(ctx, p("src"), p("in_off"), p("in_len"), n, p("sink"), p("out_off"), p("cap"), p("out_len"),
                                                   p("status"), p("detail"), C.byref(ext), mem, None)
        h, good = same_results(both(env, arrays, call), arrays, ["out_len", "status", "detail"], pos=None if dicts else "pos")
        check_decoded(h, good, plains, fail)
    finally:
        lib.lz4flex_ctx_destroy(ctx)


def encode_job(shape, seed):
    """plain blocks scattered in `src`, sinks of max_out bytes scattered in `sink`; block `fail`'s sink is one byte short of its block"""
    rng = np.random.default_rng(seed)
    n = {"n5": 5, "n9": 9, "n24-fail": 24, "big": 1}[shape]
    lens = [70000] if shape == "big" else lengths(n, rng)
    plains = [D.block(KINDS[i % 3], m, seed + i) for i, m in enumerate(lens)]
    fail = None if shape == "big" else n - 2
    caps = [O.max_out(m) for m in lens]
    if fail is not None:
        caps[fail] = len(O.compress(plains[fail])) - 1
    in_off, in_bytes = scattered(rng, lens)
    out_off, out_bytes = scattered(rng, caps)
    arrays = dict(src=buffer_of(rng, in_bytes, in_off, plains), in_off=np.array(in_off, np.uint64), in_len=np.array(lens, np.uint32),
                  sink=buffer_of(rng, out_bytes), out_off=np.array(out_off, np.uint64), cap=np.array(caps, np.uint32),
                  out_len=np.full(n, 0xDEADBEEF, np.uint32), status=np.full(n, -1, np.int32))
    return arrays, plains, fail


@pytest.mark.parametrize("shape", ["n5", "n9", "n24-fail", "big"])
def test_compress_batch(env, shape):
    lib, L, torch = env
    arrays, plains, fail = encode_job(shape, 31)
    ctx = _ctx(lib, compress_mode=1)
    try:
        def call(p, mem):
            return lib.lz4flex_compress_batch(ctx, p("src"), p("in_off"), p("in_len"), None, len(plains), p("sink"), p("out_off"), p("cap"), p("out_len"),
                                              p("status"), mem, None)
        h, good = same_results(both(env, arrays, call, big=shape == "big"), arrays, ["out_len", "status"])
        for i, g in enumerate(good):
            assert (g is None) == (i == fail), (i, h["status"])
            if g:
                comp = h["sink"][g[0]:g[0] + g[1]].tobytes()
                assert comp == O.compress(plains[i]) and O.decompress(comp, len(plains[i])) == ("ok", plains[i]), i
    finally:
        lib.lz4flex_ctx_destroy(ctx)


# ------------------------------------------------------------------------------------------------ the entries with a staging of their own
def test_decompressed_size_batch(env):
    lib, L, torch = env
    arrays, plains, _ = decode_job("n9", 41)
    n = len(plains)
    arrays["in_len"][3] -= 1                                 # cut short: the last literals ask for a byte the block does not have
    arrays.update(size=np.full(n, 0xEEEE, np.uint64), history=np.array([0, 100] * 4 + [0], np.uint32))
    ctx = _ctx(lib)
    try:
        def call(p, mem):
            return lib.lz4flex_decompressed_size_batch(ctx, p("src"), p("in_off"), p("in_len"), n, p("history"), p("size"), p("status"), mem, None)
        (rc_h, h), (rc_d, d) = both(env, arrays, call)
        assert rc_h == rc_d == 0
        assert np.array_equal(h["size"], d["size"]) and np.array_equal(h["status"], d["status"])
        assert h["status"][3] != 0 and not h["status"][:3].any()
        assert [int(v) for v in h["size"][:3]] == [len(p) for p in plains[:3]]
    finally:
        lib.lz4flex_ctx_destroy(ctx)


def test_decompress_batch_packed(env):
    lib, L, torch = env
    arrays, plains, _ = decode_job("n9", 43)
    n = len(plains)
    sizes = [len(p) for p in plains]
    sizes[7] -= 1                                            # the size it is given is one byte short: the block fails
    total = sum((s + 15) // 16 * 16 for s in sizes) + 100
    rng = np.random.default_rng(3)
    arrays.update(sizes=np.array(sizes, np.uint32), sink=buffer_of(rng, START + total), res_off=np.full(n + 1, 0xEEEE, np.uint64),
                  res_cap=np.full(n, 0xEEEE, np.uint32), work=np.zeros(int(lib.lz4flex_packed_work_size(n)) + 64, np.uint8))
    ctx = _ctx(lib)
    try:
        def call(p, mem):
            return lib.lz4flex_decompress_batch_packed(ctx, p("src"), p("in_off"), p("in_len"), n, L.SIZES_GIVEN, p("sizes"), p("sink", START), total, 16,
                                                       p("res_off"), p("res_cap"), p("out_len"), p("status"), p("detail"), p("work"), mem, None)
        res = both(env, arrays, call)
        for _, a in res:                                     # (the offsets count from the buffer the call was given)
            a["res_at"] = a["res_off"][:n] + np.uint64(START)
        h, good = same_results(res, arrays, ["res_off", "res_cap", "out_len", "status", "detail"], off="res_at")
        check_decoded(h, good, plains, 7)
    finally:
        lib.lz4flex_ctx_destroy(ctx)


def test_compress_batch_packed(env):
    lib, L, torch = env
    arrays, plains, _ = encode_job("n9", 47)
    n = len(plains)
    bound = int(lib.lz4flex_compress_packed_scratch_bound(sum(len(p) for p in plains), n, 0))
    comps = [O.compress(p) for p in plains]
    total = sum((len(c) + 7) // 8 * 8 for c in comps) - 8      # the stream ends one slot early: the last block has no room
    rng = np.random.default_rng(4)
    arrays.update(sink=buffer_of(rng, START + total + 300), res_off=np.full(n + 1, 0xEEEE, np.uint64), scratch=np.zeros(bound + 256, np.uint8),
                  work=np.zeros(int(lib.lz4flex_packed_work_size(n)) + 64, np.uint8))
    ctx = _ctx(lib, compress_mode=1)
    try:
        def call(p, mem):
            return lib.lz4flex_compress_batch_packed(ctx, p("src"), p("in_off"), p("in_len"), n, 0, p("scratch"), bound, p("sink", START), total, 8,
                                                     p("res_off"), p("out_len"), p("status"), p("work"), mem, None)
        res = both(env, arrays, call)
        for _, a in res:
            a["res_at"] = a["res_off"][:n] + np.uint64(START)
        h, good = same_results(res, arrays, ["res_off", "out_len", "status"], off="res_at")
        assert h["status"][n - 1] != 0 and not h["status"][:n - 1].any(), h["status"]
        for i, g in enumerate(good[:n - 1]):
            assert h["sink"][g[0]:g[0] + g[1]].tobytes() == comps[i] and O.decompress(comps[i], len(plains[i])) == ("ok", plains[i]), i
    finally:
        lib.lz4flex_ctx_destroy(ctx)


def test_dict_train(env):
    lib, L, torch = env
    rng = np.random.default_rng(53)
    n = 9
    samples = [D.block("json", m, i) for i, m in enumerate(lengths(n, rng))]
    in_off, in_bytes = scattered(rng, [len(s) for s in samples])
    arrays = dict(src=buffer_of(rng, in_bytes, in_off, samples), in_off=np.array(in_off, np.uint64), in_len=np.array([len(s) for s in samples], np.uint32),
                  dic=buffer_of(rng, 1000 + 64), dict_len=np.full(1, 0xEEEE, np.uint32), status=np.full(1, -1, np.int32),
                  work=np.zeros(int(lib.lz4flex_dict_train_work_size(n)) + 64, np.uint8))
    ctx = _ctx(lib)
    try:
        def call(p, mem):
            return lib.lz4flex_dict_train(ctx, p("src"), p("in_off"), p("in_len"), n, p("dic"), 1000, 64, p("dict_len"), p("status"), p("work"), mem, None)
        (rc_h, h), (rc_d, d) = both(env, arrays, call)
        assert rc_h == rc_d == 0 and h["status"][0] == d["status"][0] == 0
        m = int(h["dict_len"][0])
        assert 0 < m == int(d["dict_len"][0]) <= 1000
        assert np.array_equal(h["dic"][:m], d["dic"][:m]) and np.array_equal(h["dic"][m:], arrays["dic"][m:])
    finally:
        lib.lz4flex_ctx_destroy(ctx)


def typed_job(seed, fail):
    """blocks of whole 4-byte elements; the tmp slots of a typed compress mirror the input buffer, a typed decompress's the output buffer"""
    rng = np.random.default_rng(seed)
    lens = [m // 4 * 4 for m in lengths(9, rng)]
    plains = [D.block(KINDS[i % 3], m, seed + i) for i, m in enumerate(lens)]
    in_off, in_bytes = scattered(rng, lens)
    return rng, lens, plains, in_off, in_bytes


def test_filter_batch(env):
    lib, L, torch = env
    rng, lens, plains, in_off, in_bytes = typed_job(59, None)
    out_off, out_bytes = scattered(rng, lens)
    arrays = dict(src=buffer_of(rng, in_bytes, in_off, plains), in_off=np.array(in_off, np.uint64), in_len=np.array(lens, np.uint32),
                  sink=buffer_of(rng, out_bytes), out_off=np.array(out_off, np.uint64))
    ctx = _ctx(lib)
    try:
        def call(p, mem):
            return lib.lz4flex_filter_batch(ctx, p("src"), p("in_off"), p("in_len"), 9, p("sink"), p("out_off"), L.FILTER_SHUFFLE, 4, 0, mem, None)
        h, good = same_results(both(env, arrays, call), arrays, [], length="in_len", status=None)
        for i, (o, m) in enumerate(good):                    # byte k of element e goes to k * elements + e
            assert h["sink"][o:o + m].tobytes() == u8(plains[i]).reshape(-1, 4).T.tobytes(), i
    finally:
        lib.lz4flex_ctx_destroy(ctx)


def test_compress_and_decompress_batch_typed(env):
    lib, L, torch = env
    rng, lens, plains, in_off, in_bytes = typed_job(61, 7)
    n = 9
    shuffled = [u8(p).reshape(-1, 4).T.tobytes() for p in plains]
    comps = [O.compress(s) for s in shuffled]
    caps = [O.max_out(m) for m in lens]
    caps[7] = len(comps[7]) - 1
    out_off, out_bytes = scattered(rng, caps)
    arrays = dict(src=buffer_of(rng, in_bytes, in_off, plains), in_off=np.array(in_off, np.uint64), in_len=np.array(lens, np.uint32),
                  sink=buffer_of(rng, out_bytes), out_off=np.array(out_off, np.uint64), cap=np.array(caps, np.uint32),
                  out_len=np.full(n, 0xDEADBEEF, np.uint32), status=np.full(n, -1, np.int32), tmp=np.zeros(in_bytes + 64, np.uint8))
    ctx = _ctx(lib, compress_mode=1)
    try:
        def call(p, mem):
            return lib.lz4flex_compress_batch_typed(ctx, p("src"), p("in_off"), p("in_len"), n, p("sink"), p("out_off"), p("cap"), p("out_len"), p("status"),
                                                    L.FILTER_SHUFFLE, 4, p("tmp"), p("in_off"), mem, None)
        h, good = same_results(both(env, arrays, call), arrays, ["out_len", "status"])
        for i, g in enumerate(good):
            assert (g is None) == (i == 7), (i, h["status"])
            if g:
                assert h["sink"][g[0]:g[0] + g[1]].tobytes() == comps[i] and O.decompress(comps[i], lens[i]) == ("ok", shuffled[i]), i
        # ... and back: the blocks the oracle wrote, a sink one byte short for block 7
        c_off, c_bytes = scattered(rng, [len(c) for c in comps])
        dcaps = [m + 5 for m in lens]
        dcaps[7] = lens[7] - 1
        d_off, d_bytes = scattered(rng, dcaps)
        back = dict(src=buffer_of(rng, c_bytes, c_off, comps), in_off=np.array(c_off, np.uint64), in_len=np.array([len(c) for c in comps], np.uint32),
                    sink=buffer_of(rng, d_bytes), out_off=np.array(d_off, np.uint64), cap=np.array(dcaps, np.uint32),
                    out_len=np.full(n, 0xDEADBEEF, np.uint32), status=np.full(n, -1, np.int32), detail=np.full(2 * n, 0xEE, np.uint64),
                    tmp=np.zeros(d_bytes + 64, np.uint8))

        def call_back(p, mem):
            return lib.lz4flex_decompress_batch_typed(ctx, p("src"), p("in_off"), p("in_len"), n, p("sink"), p("out_off"), p("cap"), p("out_len"),
                                                      p("status"), p("detail"), L.FILTER_SHUFFLE, 4, p("tmp"), p("out_off"), mem, None)
        h, good = same_results(both(env, back, call_back), back, ["out_len", "status", "detail"])
        check_decoded(h, good, plains, 7)
    finally:
        lib.lz4flex_ctx_destroy(ctx)


def test_fit_batch_and_compress_batch_fit(env):
    lib, L, torch = env
    rng = np.random.default_rng(67)
    n = 9
    lens = lengths(n, rng)
    plains = [D.block(KINDS[i % 3], m, 67 + i) for i, m in enumerate(lens)]
    comps = [O.compress(p) for p in plains]
    caps = [max(1, len(c) * 2 // 3) for c in comps]           # every block is cut; a capacity of 0 is the one way to fail
    caps[7] = 0
    src_off, src_bytes = scattered(rng, lens)
    blk_off, blk_bytes = scattered(rng, [len(c) for c in comps])
    out_off, out_bytes = scattered(rng, caps)
    arrays = dict(src=buffer_of(rng, src_bytes, src_off, plains), in_off=np.array(src_off, np.uint64), in_len=np.array(lens, np.uint32),
                  blk=buffer_of(rng, blk_bytes, blk_off, comps), blk_off=np.array(blk_off, np.uint64), blk_len=np.array([len(c) for c in comps], np.uint32),
                  sink=buffer_of(rng, out_bytes), out_off=np.array(out_off, np.uint64), cap=np.array(caps, np.uint32),
                  out_len=np.full(n, 0xDEADBEEF, np.uint32), used=np.full(n, 0xDEADBEEF, np.uint32), status=np.full(n, -1, np.int32),
                  scratch=np.zeros(sum(O.max_out(m) for m in lens) + 256, np.uint8), work=np.zeros(int(lib.lz4flex_compress_fit_work_size(n)) + 64, np.uint8))
    ctx = _ctx(lib, compress_mode=1)
    try:
        def fit(p, mem):
            return lib.lz4flex_fit_batch(ctx, p("blk"), p("blk_off"), p("blk_len"), p("src"), p("in_off"), p("in_len"), n, p("sink"), p("out_off"), p("cap"),
                                         p("out_len"), p("used"), p("status"), mem, None)

        def compress_fit(p, mem):
            return lib.lz4flex_compress_batch_fit(ctx, p("src"), p("in_off"), p("in_len"), n, p("scratch"), len(arrays["scratch"]) - 256, p("sink"), p("out_off"),
                                                  p("cap"), p("out_len"), p("used"), p("status"), p("work"), mem, None)
        for call in (fit, compress_fit):
            h, good = same_results(both(env, arrays, call), arrays, ["out_len", "used", "status"])
            for i, g in enumerate(good):
                assert (g is None) == (i == 7), (call.__name__, i, h["status"])
                if g:                                        # a block of at most cap bytes that decodes to the first in_used bytes
                    m = int(h["used"][i])
                    assert g[1] <= caps[i] and O.decompress(h["sink"][g[0]:g[0] + g[1]].tobytes(), m) == ("ok", plains[i][:m]), (call.__name__, i)
    finally:
        lib.lz4flex_ctx_destroy(ctx)
