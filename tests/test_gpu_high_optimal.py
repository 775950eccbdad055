"""GPU (-m gpu): compress_mode 2 ("high") under "compress_parse" 1, the optimal parse (lz4_compress_high.hip, step 3 1/2) through the C
ABI.  The kernels must reproduce the scalar definition (tests/sim/high_optimal_model.c) byte for byte: the plain form, the dictionary
form through every entry that takes dictionaries, the history form; in host and device memory, at depths 1, 16 and 256; with the setting
at 0 the bytes are what they were."""
import concurrent.futures
import ctypes as C
import random

import numpy as np
import pytest

import fit_model as F
import hc_model as H
import hc_optimal_model as P
import oracle_api as O
from test_gpu_high_dict import encode as dict_encode
from test_gpu_high_mode import log_blocks, run_batch
from test_gpu_high_mode_linked import Batch, run as linked_run, slots, walk as frame_walk

pytestmark = pytest.mark.gpu

DEPTHS = (1, 16, 256)
BEST = (4, 18, 19, 35, 36, 37, 273, 274)
NO_DICT = 0xFFFFFFFF


def J():
    return O.fixture_plain("compression_66k_JSON")


def T():
    return O.fixture_plain("compression_65k")


_blocks = {}


def blocks(chunk):
    """[(name, block)] for the form whose first chunk has `chunk` positions (65 536: the plain form, 32 768: with a dictionary)"""
    if chunk not in _blocks:
        rnd = random.Random(31)
        R = rnd.randbytes
        j, t = J(), T()
        out = [("text %d" % n, (t * 4)[:n]) for n in (0, 11, 12, 13, 2047, 2048, 2049, 4097)]
        out += [("JSON %d" % n, (j * 4)[:n]) for n in (chunk + 11, chunk + 12)]
        for L in BEST:                                           # a phrase of L bytes twice, different bytes around both copies
            ph = R(L)
            out.append(("best %d" % L, R(300) + b"\x01" + ph + b"\x02" + R(97) + b"\x03" + ph + b"\x04" + R(40)))
        ph = R(40)
        for room in (2, 19):                                     # the second copy starts `room` positions in front of 2 048
            out.append(("cross %d" % room, ph + R(2048 - room - 40) + ph + R(200)))
        ph = R(300)
        out.append(("chunk end", ph + R(chunk - 136 - 300) + ph + R(500)))      # ... and 136 in front of the chunk's end
        out += [("zeros", bytes(200000)), ("period 2", b"ab" * 35000), ("random", R(5000)), ("random 70000", R(70000)),
                ("compression_34k", O.fixture_plain("compression_34k")), ("compression_65k", t), ("compression_66k_JSON", j)]
        _blocks[chunk] = out
    return _blocks[chunk]


def dicts_for(n):
    """a dictionary per block, in rotation: text, JSON, none, 3 bytes, zeros, more than 32 KiB"""
    j, t = J(), T()
    pool = (t[1000:30000], j[:32768], b"", t[:3], bytes(5000), j[100:40100])
    return [pool[k % len(pool)] for k in range(n)]


def model(data, d=b"", depth=16, parse=1):
    return P.compress(data, d[-32768:] if len(d) >= 4 else b"", depth, parse)


def test_the_blocks_are_what_they_say():
    """(the model alone) the best lengths, the rooms and the chunk's end"""
    for chunk in (65536, 32768):
        named = dict(blocks(chunk))
        assert len(named) == len(blocks(chunk)) <= 36 and max(len(b) for b in named.values()) <= 200000
        for L in BEST:
            _, best_len, _, pick = P.trace(named["best %d" % L], b"", 16, 1)
            assert max(best_len) == L and best_len.count(L) == 1 and pick[best_len.index(L)] == L
        for room in (2, 19):
            _, best_len, _, pick = P.trace(named["cross %d" % room], b"", 16, 1)
            assert best_len[2048 - room] == 40
            # (behind the segment's end everything is free: 2 literals are cheaper than the match, 19 are not)
            assert pick[2048 - room] == (0 if room == 2 else 40)
        d = b"" if chunk == 65536 else T()[1000:30000]
        _, best_len, _, _ = P.trace(named["chunk end"], d, 16, 1)
        assert best_len[chunk - 136] == 136
        _, best_len, _, _ = P.trace(named["random"], b"", 16, 1)
        assert max(best_len) == 0


@pytest.fixture(scope="module")
def env():
    from lz4_flex_amd import _lib
    lib = _lib.load()
    assert lib.lz4flex_device_count() >= 1
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
    for key, v in ((b"compress_mode", 2), (b"compress_depth", 16), (b"compress_parse", 1)):
        assert lib.lz4flex_set_tuning(ctx, key, v) == 0
    yield lib, ctx
    lib.lz4flex_ctx_destroy(ctx)


def tune(env, **kv):
    lib, ctx = env
    for key, v in kv.items():
        assert lib.lz4flex_set_tuning(ctx, key.encode(), v) == 0, key


def check(names, want, res):
    """every slot holds the wanted bytes and every byte outside them is untouched (0xEE)"""
    out, out_off, out_len, st = res
    image = np.full(out.size, 0xEE, dtype=np.uint8)
    for k, m in enumerate(want):
        assert int(st[k]) == 0 and int(out_len[k]) == len(m), (names[k], int(st[k]), int(out_len[k]), len(m))
        image[int(out_off[k]):int(out_off[k]) + len(m)] = np.frombuffer(m, dtype=np.uint8)
    bad = np.flatnonzero(image != out)
    if bad.size:
        k = int(np.searchsorted(out_off, bad[0], side="right")) - 1
        raise AssertionError("first difference at output byte %d: block %r, byte %d of its slot" % (bad[0], names[k], bad[0] - int(out_off[k])))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_plain_form_equals_model(env, depth, device):
    from lz4_flex_amd import _lib as L
    tune(env, compress_depth=depth)
    try:
        names, data = zip(*blocks(65536))
        res = run_batch(env[0], env[1], list(data), L.MEM_DEVICE if device else L.MEM_HOST)
        check(names, [model(b, b"", depth) for b in data], res)
        if depth == 16 and not device:
            for b, comp in zip(data, slots(res)):
                assert O.decompress(comp, len(b)) == ("ok", b)
    finally:
        tune(env, compress_depth=16)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_ex_equals_model(env, depth, device):
    tune(env, compress_depth=depth, compress_high_dict=1)
    try:
        names, data = zip(*blocks(32768))
        ds = dicts_for(len(data))
        res = dict_encode(env, "ex", device, data, dicts=ds)
        check(names, [model(b, d, depth) for b, d in zip(data, ds)], res)
        if depth == 16 and not device:
            for b, d, comp in zip(data, ds, slots(res)):
                assert O.decompress(comp, len(b), dict_data=d or None) == ("ok", b)
    finally:
        tune(env, compress_depth=16, compress_high_dict=0)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_dict_set_equals_model(env, depth, device):
    from lz4_flex_amd import block
    tune(env, compress_depth=depth, compress_high_dict=1)
    try:
        names, data = zip(*blocks(32768))
        ds = dicts_for(len(data))
        pool = sorted(set(d for d in ds if d), key=len)
        ids = [pool.index(d) if d else NO_DICT for d in ds]
        with block.DictSet(pool, ctx=env[1]) as dset:
            res = dict_encode(env, "dict_set", device, data, ids=ids, dset=dset)
        check(names, [model(b, d, depth) for b, d in zip(data, ds)], res)
    finally:
        tune(env, compress_depth=16, compress_high_dict=0)


@pytest.mark.parametrize("digest", [1, 0])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_shared_dict_equals_model(env, depth, device, digest):
    tune(env, compress_depth=depth, compress_high_dict=1, compress_high_digest=digest)
    try:
        names, data = zip(*blocks(32768))
        d = T()[1000:30000]
        res = dict_encode(env, "shared_dict", device, data, shared=d)
        check(names, [model(b, d, depth) for b in data], res)
    finally:
        tune(env, compress_depth=16, compress_high_dict=0, compress_high_digest=1)


def history_batch():
    """every block of the dictionary form's list behind its dictionary as its own stream's history, and four without history bits"""
    b = Batch()
    named = blocks(32768)
    for (name, data), d in zip(named, dicts_for(len(named))):
        s = b.stream(d + data)
        b.block(s, len(d), len(data), len(d))
    for name, data in blocks(65536)[-4:]:
        b.block(b.stream(data), 0, len(data), 0)
    return b


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_history_form_equals_model(env, depth, device):
    tune(env, compress_depth=depth, compress_high_linked=1)
    try:
        b = history_batch()
        res = linked_run(env, b, device)
        want = [P.block(b.streams[s], at, n, fl >> 8, depth, 1) for s, at, n, fl in b.blocks]
        check([blk[1:] for blk in b.blocks], want, res)
        if depth == 16 and not device:
            for k, comp in enumerate(slots(res)):
                assert O.decompress(comp, b.blocks[k][2], dict_data=b.history(k) or None) == ("ok", b.plain(k)), k
    finally:
        tune(env, compress_depth=16, compress_high_linked=0)


def test_more_blocks_than_workgroups_and_alone(env):
    """more blocks than persistent workgroups; a block's bytes are the same alone and among 300"""
    from lz4_flex_amd import _lib as L
    many = log_blocks(env[0])
    res = run_batch(env[0], env[1], many, L.MEM_DEVICE)
    check(list(range(len(many))), [model(b) for b in many], res)
    j = (J() * 4)[:70000]
    crowd = many[:150] + [j] + many[150:299]
    assert len(crowd) == 300
    among = slots(run_batch(env[0], env[1], crowd, L.MEM_DEVICE))[150]
    alone = slots(run_batch(env[0], env[1], [j], L.MEM_DEVICE))[0]
    assert among == alone == model(j)


def test_every_decoder_reads_the_blocks(env):
    from lz4_flex_amd import block
    lib, ctx = env
    data = [b for _, b in blocks(65536)]
    comp = [model(b) for b in data]
    src = np.frombuffer(b"".join(comp), dtype=np.uint8)
    in_len = np.array([len(c) for c in comp], dtype=np.uint32)
    in_off = (np.cumsum(in_len.astype(np.uint64)) - in_len).astype(np.uint64)
    cap = np.array([len(b) for b in data], dtype=np.uint32)
    out_off = (np.cumsum(cap.astype(np.uint64)) - cap).astype(np.uint64)
    plain = np.frombuffer(b"".join(data), dtype=np.uint8)
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


def test_setting_0_and_back_to_0(env):
    from lz4_flex_amd import _lib as L
    names, data = zip(*blocks(65536)[-12:])
    lazy = [H.compress(b, 16) for b in data]
    try:
        tune(env, compress_parse=0)
        check(names, lazy, run_batch(env[0], env[1], list(data), L.MEM_DEVICE))
        tune(env, compress_parse=1)
        check(names, [model(b) for b in data], run_batch(env[0], env[1], list(data), L.MEM_DEVICE))
        tune(env, compress_parse=0)
        check(names, lazy, run_batch(env[0], env[1], list(data), L.MEM_DEVICE))
        # the other modes do not read it
        tune(env, compress_mode=1)
        exact = slots(run_batch(env[0], env[1], list(data), L.MEM_DEVICE))
        tune(env, compress_parse=1)
        assert slots(run_batch(env[0], env[1], list(data), L.MEM_DEVICE)) == exact
        assert exact != lazy
    finally:
        tune(env, compress_mode=2, compress_parse=1)


def test_the_environment_variable():
    """LZ4FLEX_HIGH_PARSE=optimal is a new context's "compress_parse" (a fresh process: the variable is read when a context is made;
    without it the setting is 0: tests/test_high_optimal_api.py)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import ctypes as C\nfrom lz4_flex_amd import _lib\nlib = _lib.load()\nctx = C.c_void_p()\n"
            "assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0\nprint(lib.lz4flex_get_tuning(ctx, b'compress_parse'))\n")
    env = dict(os.environ, PYTHONPATH=root, LZ4FLEX_HIGH_PARSE="optimal")
    assert subprocess.check_output([sys.executable, "-c", code], env=env, cwd=root).decode().strip() == "1"


# ------------------------------------------------------------------------------------------- this thread's default context
_worker = concurrent.futures.ThreadPoolExecutor(max_workers=1)


def in_worker(fn):
    """the test runs in this module's worker thread with that thread's default context (the scalar calls, the frame layer) in mode high
    with the optimal parse: the main thread's default context, which other files' tests share, sees none of it"""
    def body():
        from lz4_flex_amd import block
        block.set_compress_mode("high")
        block.set_compress_depth(16)
        block.set_compress_parse("optimal")
        try:
            return fn(block)
        finally:
            block.set_compress_mode("fast")
            block.set_compress_parse("lazy")
            block.set_compress_high_linked(False)

    def run():
        return _worker.submit(body).result()

    run.__name__, run.__doc__, run.__module__ = fn.__name__, fn.__doc__, fn.__module__
    return run


@in_worker
def test_scalar_packed_and_fit_calls(block):
    j = J()
    data = (j * 4)[:98305]
    assert block.compress(data) == model(data)
    assert block.compress(b"") == model(b"")
    out = bytearray(block.get_maximum_output_size(len(data)))
    n = block.compress_into_with_table(data, out, block.CompressTable.small())      # (the table context takes the default one's settings)
    assert bytes(out[:n]) == model(data)
    parts = [j[:5000], (j * 2)[100:100 + 70000], b"", j[7:4103]]
    src = np.frombuffer(b"".join(parts), dtype=np.uint8)
    in_len = np.array([len(b) for b in parts], dtype=np.uint32)
    in_off = (np.cumsum(in_len.astype(np.uint64)) - in_len).astype(np.uint64)
    out = np.zeros(sum(O.max_out(len(b)) + 4 for b in parts), dtype=np.uint8)
    out_off, out_len, st = block.compress_batch_packed(src, in_off, in_len, out, prepend_size=True)
    assert not st.any()
    for k, b in enumerate(parts):
        assert bytes(out[int(out_off[k]):int(out_off[k]) + int(out_len[k])]) == len(b).to_bytes(4, "little") + model(b), k
    # fit: the model's block cut to the capacity by the fit rule
    caps = [1000, 3000, 16, 5000]
    cap_off = (np.cumsum(caps) - np.array(caps)).astype(np.uint64)
    out = np.zeros(sum(caps), dtype=np.uint8)
    out_len, used, st = block.compress_batch_fit(src, in_off, in_len, out, cap_off, caps)
    for k, b in enumerate(parts):
        want, want_used, want_st = F.fit(model(b), b, caps[k])
        assert (int(st[k]), int(used[k])) == (want_st, want_used), k
        assert bytes(out[int(cap_off[k]):int(cap_off[k]) + int(out_len[k])]) == want, k


@in_worker
def test_independent_frame(block):
    from lz4_flex_amd import frame
    data = (J() * 4)[:3 * 65536 + 17]
    fi = frame.FrameInfo(block_size=frame.BlockSize.Max64KB, block_mode=frame.BlockMode.Independent)
    f = frame.compress_frame(data, fi)
    assert O.frame_decompress(f, len(data))[:2] == (0, data)
    want = []
    for at in range(0, len(data), 65536):
        raw = data[at:at + 65536]
        m = model(raw)
        want.append((m, False) if len(m) < len(raw) else (raw, True))
    assert frame_walk(f, want, False) == want
    assert frame.compress_frames([data, data[:70000]], fi)[0] == f
    block.set_compress_parse("lazy")
    assert len(f) < len(frame.compress_frame(data, fi))


@in_worker
def test_linked_frame(block):
    from lz4_flex_amd import frame
    block.set_compress_high_linked(True)
    data = J() + T()
    fi = frame.FrameInfo(block_size=frame.BlockSize.Max64KB, block_mode=frame.BlockMode.Linked)
    f = frame.compress_frame(data, fi)
    assert O.frame_decompress(f, len(data))[:2] == (0, data)
    assert O.c_frame_decompress(f, len(data)) == data
    want = []
    for at in range(0, len(data), 65536):
        n = min(65536, len(data) - at)
        m = P.block(data, at, n, at, 16, 1)
        want.append((m, False) if len(m) < n else (data[at:at + n], True))
    assert frame_walk(f, want, False) == want
