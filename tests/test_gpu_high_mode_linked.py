"""GPU (-m gpu): compress_mode 2 ("high") over a stream's history ("compress_high_linked" 1; lz4_compress_high.hip, the history form)
through the C ABI.  A block with LZ4FLEX_BLOCK_HISTORY(h) gets the bytes of the scalar definition (tests/sim/high_dict_model.c with the
h bytes in front of the block as its dictionary; tests/hc_linked_model.py) -- in raw batches in host and device memory, through the
frame layer's three encoders and the command line; with the setting at 0 nothing changes.

The file's name sorts it behind test_gpu_high_mode.py on purpose.  test_dictionary_entries_give_mode_0_bytes there compares two
consecutive mode 0 calls of lz4flex_compress_batch_ex, and mode 0's bytes for its 100-byte block behind a 40 000-byte dictionary are
not the same from call to call (22, 29 and 35 bytes were seen in one process, settling after two calls): they follow what earlier
launches of the process left in device memory.  With this file in front of it that test failed; the throughput encoder is not this
file's subject and is left as it is ("Known").  The tests here that use a default context run in a thread of their own."""
import concurrent.futures
import ctypes as C
import inspect
import io
import random

import numpy as np
import pytest

import hc_linked_model as K
import hc_model as H
import oracle_api as O
from test_high_dict_model import sequences

pytestmark = pytest.mark.gpu

CANARY = 16
EDGE_H = (0, 1, 3, 4, 5, 11, 12, 4095, 32767, 32768, 32769, 40000)
EDGE_LEN = (1273, 1273, 1273, 1269, 1268, 1265, 1264, 767, 726, 726, 726, 726)
LENGTHS = (0, 1, 11, 12, 13, 17, 64, 32767, 32768, 32769, 65536 + 17, 3 * 32768 + 5)


def J():
    return O.fixture_plain("compression_66k_JSON")


def T():
    return O.fixture_plain("compression_65k")


def log_1m():
    from lz4_flex_amd import workloads
    return bytes(workloads.log_stream(0, 1 << 20).numpy())


class Batch:
    """streams side by side in one input buffer (each from a 4-aligned start) and blocks cut out of them: (stream, at, n, flag word)"""

    def __init__(self):
        self.streams, self.blocks = [], []

    def stream(self, data):
        self.streams.append(bytes(data))
        return len(self.streams) - 1

    def block(self, s, at, n, h, bits=0):
        assert 0 <= h <= at and at + n <= len(self.streams[s])
        self.blocks.append((s, at, n, (h << 8) | bits))

    def plain(self, k):
        s, at, n, _ = self.blocks[k]
        return self.streams[s][at:at + n]

    def history(self, k):
        s, at, _, fl = self.blocks[k]
        return self.streams[s][at - (fl >> 8):at]

    def model(self, k, depth, linked=True):
        s, at, n, fl = self.blocks[k]
        return K.block(self.streams[s], at, n, (fl >> 8) if linked else 0, depth)

    def arrays(self):
        base, at = [], 0
        for s in self.streams:
            base.append(at)
            at += (len(s) + 3) // 4 * 4 + 4
        buf = np.zeros(at + 64, dtype=np.uint8)
        for b, s in zip(base, self.streams):
            buf[b:b + len(s)] = np.frombuffer(s, dtype=np.uint8)
        in_off = np.array([base[s] + a for s, a, _, _ in self.blocks], dtype=np.uint64)
        in_len = np.array([n for _, _, n, _ in self.blocks], dtype=np.uint32)
        flags = np.array([fl for _, _, _, fl in self.blocks], dtype=np.uint32)
        return buf, in_off, in_len, flags


_edge = []


def edge_batch():
    """the history's edges, every block length behind 32 KiB, every pair of alignments, a match out of the history into the block, a
    run of one byte, blocks without history bits between them"""
    if not _edge:
        b = Batch()
        j, t = J(), T()
        sj = b.stream(j)
        for h in EDGE_H:
            b.block(sj, 40000, 5000, h)
        s4 = [b.stream(j * 4), b.stream(t * 4)]
        for i, n in enumerate(LENGTHS):
            b.block(s4[i & 1], 32768, n, 32768)
        b.block(s4[0], 40000, 3 * 32768 + 5, 40000, bits=3)          # (frame bits beside the history: not read)
        # (in_off - h) & 3 and in_off & 3: the streams start at multiples of 4
        for a in range(4):
            for r in range(4):
                b.block(sj, 40000 + a, 3000, 5000 + ((a - r) & 3))
        rnd = random.Random(5)
        d = bytes(rnd.getrandbits(8) for _ in range(5000))
        sm = b.stream(d + d[-40:] + d[-40:] + bytes(rnd.getrandbits(8) for _ in range(30)))
        b.block(sm, 5000, 110, 5000)
        b.match_block = len(b.blocks) - 1
        sz = b.stream(b"\x07" * (32768 + 40000))
        b.block(sz, 32768, 40000, 32768)
        for bits in (0, 1, 3, 2):
            b.block(sj, 1000, 5000, 0, bits=bits)
        b.block(s4[1], 70000, 70000, 0, bits=1)
        _edge.append(b)
    return _edge[0]


_many = {}


def many_batch(lib):
    """more blocks than persistent workgroups: 2 G + 1 small ones cut from one stream, one after the other"""
    g = lib.lz4flex_get_tuning(None, b"compress_workgroups") // 2
    if g not in _many:
        b = Batch()
        log = log_1m()
        s = b.stream(log)
        rnd = random.Random(7)
        at = 0
        for _ in range(2 * g + 1):
            n = rnd.randint(700, 2000)
            assert at + n <= len(log)
            b.block(s, at, n, min(at, 32768))
            at += n
        _many[g] = b
    return _many[g]


@pytest.fixture(scope="module")
def env():
    from lz4_flex_amd import _lib
    lib = _lib.load()
    assert lib.lz4flex_device_count() >= 1
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
    for key, v in ((b"compress_mode", 2), (b"compress_high_linked", 1), (b"compress_depth", 16)):
        assert lib.lz4flex_set_tuning(ctx, key, v) == 0
    yield lib, ctx
    lib.lz4flex_ctx_destroy(ctx)


def tune(env, **kv):
    lib, ctx = env
    for key, v in kv.items():
        assert lib.lz4flex_set_tuning(ctx, key.encode(), v) == 0, key


def run(env, batch, device, caps=None):
    """one lz4flex_compress_batch over the batch with its flag words: (the whole output buffer, out_off, out_len, status); the
    output slots have `caps` bytes (default: the bound) and CANARY bytes of 0xEE in front of and behind each"""
    from lz4_flex_amd import _lib as L
    lib, ctx = env
    buf, in_off, in_len, flags = batch.arrays()
    n = len(in_len)
    cap = np.array([O.max_out(int(v)) for v in in_len] if caps is None else caps, dtype=np.uint32)
    out_off = (np.cumsum(cap.astype(np.uint64) + CANARY) - cap).astype(np.uint64)
    out = np.full(int(out_off[-1] + cap[-1]) + CANARY, 0xEE, dtype=np.uint8)
    out_len, st = np.zeros(n, dtype=np.uint32), np.full(n, -1, dtype=np.int32)
    if device:
        import torch
        dev = torch.device("cuda", 0)
        tt = lambda a, dt: torch.from_numpy(a.view(dt)).to(dev)      # noqa: E731
        d = [tt(buf, np.uint8), tt(in_off, np.int64), tt(in_len, np.int32), tt(flags, np.int32), tt(out, np.uint8), tt(out_off, np.int64),
             tt(cap, np.int32), tt(out_len, np.int32), tt(st, np.int32)]
        p = [C.c_void_p(x.data_ptr()) for x in d]
        rc = lib.lz4flex_compress_batch(ctx, p[0], p[1], p[2], p[3], n, p[4], p[5], p[6], p[7], p[8], L.MEM_DEVICE, None)
        assert rc == 0, L.last_error()
        torch.cuda.synchronize()
        return d[4].cpu().numpy(), out_off, d[7].cpu().numpy().view(np.uint32), d[8].cpu().numpy()
    p = [C.c_void_p(a.ctypes.data) for a in (buf, in_off, in_len, flags, out, out_off, cap, out_len, st)]
    rc = lib.lz4flex_compress_batch(ctx, p[0], p[1], p[2], p[3], n, p[4], p[5], p[6], p[7], p[8], L.MEM_HOST, None)
    assert rc == 0, L.last_error()
    return out, out_off, out_len, st


def check(batch, depth, res, refused=(), linked=True):
    """every slot holds the model's bytes (a refused one: OUTPUT_TOO_SMALL and nothing) and every byte outside them is untouched"""
    out, out_off, out_len, st = res
    want = np.full(out.size, 0xEE, dtype=np.uint8)
    for k in range(len(batch.blocks)):
        if k in refused:
            assert (int(st[k]), int(out_len[k])) == (1, 0), k          # LZ4FLEX_E_OUTPUT_TOO_SMALL
            continue
        m = batch.model(k, depth, linked)
        assert int(st[k]) == 0 and int(out_len[k]) == len(m), (k, batch.blocks[k][1:], int(st[k]), int(out_len[k]), len(m))
        want[int(out_off[k]):int(out_off[k]) + len(m)] = np.frombuffer(m, dtype=np.uint8)
    bad = np.flatnonzero(want != out)
    if bad.size:
        k = int(np.searchsorted(out_off, bad[0], side="right")) - 1
        raise AssertionError("first difference at output byte %d: block %d %r, byte %d of its slot"
                             % (bad[0], k, batch.blocks[k][1:], bad[0] - int(out_off[k])))


def slots(res):
    out, out_off, out_len, _ = res
    return [bytes(out[int(o):int(o) + int(n)]) for o, n in zip(out_off, out_len)]


def test_the_edge_batch_is_what_it_says():
    """(the model alone) the edge list's sizes; the match that starts in the history and runs into the block"""
    b = edge_batch()
    assert [len(b.model(k, 16)) for k in range(len(EDGE_H))] == list(EDGE_LEN)
    assert sequences(b.model(b.match_block, 16))[0] == (0, 40, 80)
    seen = {((int(o) - (fl >> 8)) & 3, int(o) & 3) for o, fl in zip(b.arrays()[1], b.arrays()[3]) if fl >> 8}
    assert len(seen) == 16


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("depth", [1, 16, 256])
def test_raw_batch_equals_model(env, depth, device):
    tune(env, compress_depth=depth)
    try:
        b = edge_batch()
        res = run(env, b, device)
        check(b, depth, res)
        if depth == 16 and not device:
            # the oracle decodes every block behind its stream
            for k, comp in enumerate(slots(res)):
                s, at, n, fl = b.blocks[k]
                d = b.streams[s][max(0, at - 65536):at] if fl >> 8 else b""
                assert O.decompress(comp, n, dict_data=d or None) == ("ok", b.plain(k)), k
    finally:
        tune(env, compress_depth=16)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_more_blocks_than_workgroups(env, device):
    tune(env, compress_depth=16)
    b = many_batch(env[0])
    refused = set(range(6, len(b.blocks), 7))
    caps = [O.max_out(n) - (1 if k in refused else 0) for k, (_, _, n, _) in enumerate(b.blocks)]
    res = run(env, b, device, caps=caps)
    check(b, 16, res, refused)
    if not device:
        # the blocks lie one after the other in their stream: the oracle decodes the concatenation, block behind block
        full = run(env, b, False)
        check(b, 16, full)
        got = b""
        for k, comp in enumerate(slots(full)):
            rc, piece = O.decompress(comp, b.blocks[k][2], dict_data=got[-65536:] or None)
            assert rc == "ok", k
            got += piece
        assert got == b.streams[0][:len(got)] and len(got) == sum(n for _, _, n, _ in b.blocks)


def history_only(b):
    """the blocks of a batch that have history bits, as (dictionary, block) pairs"""
    ks = [k for k in range(len(b.blocks)) if b.blocks[k][3] >> 8]
    return ks, [b.history(k) for k in ks], [b.plain(k) for k in ks]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_ex_with_the_history_as_dictionary_gives_the_same_bytes(env, device):
    from test_gpu_high_dict import encode
    tune(env, compress_depth=16, compress_high_dict=1)
    try:
        b = edge_batch()
        ks, dicts, blocks = history_only(b)
        ex = encode(env, "ex", device, blocks, dicts=dicts)
        assert not ex[3].any()
        mine = slots(run(env, b, device))
        assert [bytes(ex[0][int(o):int(o) + int(n)]) for o, n in zip(ex[1], ex[2])] == [mine[k] for k in ks]
    finally:
        tune(env, compress_high_dict=0)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_ex_still_refuses_a_dictionary_with_history_bits(env, device):
    from lz4_flex_amd import _lib as L
    from test_gpu_high_dict import check as ex_check, encode
    tune(env, compress_depth=16, compress_high_dict=1)
    try:
        j = J()
        blocks = [j[40000:44096], j[40000:44096], j[50000:50100], j[41000:45000]]
        dicts = [j[:32768], j[:32768], b"", j[:4096]]
        res = encode(env, "ex", device, blocks, dicts=dicts, flags=[0, 32768 << 8, 32768 << 8, 1], in_shift=40000)
        ex_check(blocks, dicts, 16, res, refused={1: L.E_INVALID_ARG, 3: L.E_INVALID_ARG})
    finally:
        tune(env, compress_high_dict=0)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_setting_0_ignores_the_history(env, device):
    tune(env, compress_depth=16, compress_high_linked=0)
    try:
        b = edge_batch()
        check(b, 16, run(env, b, device), linked=False)
    finally:
        tune(env, compress_high_linked=1)


def test_host_batch_refuses_a_history_in_front_of_the_buffer(env):
    """MEM_HOST: h <= in_off[i], in mode 2 as in mode 0"""
    from lz4_flex_amd import _lib as L
    lib, ctx = env
    j = J()
    buf = np.frombuffer(j, dtype=np.uint8)
    in_off, in_len, flags = np.array([100], dtype=np.uint64), np.array([1000], dtype=np.uint32), np.array([101 << 8], dtype=np.uint32)
    cap = np.array([O.max_out(1000)], dtype=np.uint32)
    out, out_off = np.zeros(int(cap[0]), dtype=np.uint8), np.zeros(1, dtype=np.uint64)
    out_len, st = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.int32)
    p = [C.c_void_p(a.ctypes.data) for a in (buf, in_off, in_len, flags, out, out_off, cap, out_len, st)]
    assert lib.lz4flex_compress_batch(ctx, p[0], p[1], p[2], p[3], 1, p[4], p[5], p[6], p[7], p[8], L.MEM_HOST, None) == -L.E_INVALID_ARG
    flags[0] = 100 << 8
    assert lib.lz4flex_compress_batch(ctx, p[0], p[1], p[2], p[3], 1, p[4], p[5], p[6], p[7], p[8], L.MEM_HOST, None) == 0
    assert bytes(out[:int(out_len[0])]) == K.block(j, 100, 1000, 100, 16)


# ---------------------------------------------------------------------------------------------------------------- frames
_worker = concurrent.futures.ThreadPoolExecutor(max_workers=1)


def high_linked(fn):
    """The test runs in this module's one worker thread, with that thread's default context (the frame layer, the scalar calls) in
    mode high with the setting on, and is handed lz4_flex_amd.block as its first argument.  A default context belongs to its thread:
    the main thread's, which the tests of the other files share, sees none of these calls -- neither settings nor what the launches
    leave in its workspace and staging buffers."""
    def body(*args, **kw):
        from lz4_flex_amd import block
        block.set_compress_mode("high")
        block.set_compress_depth(16)
        block.set_compress_high_linked(True)
        try:
            return fn(block, *args, **kw)
        finally:
            block.set_compress_mode("fast")
            block.set_compress_high_linked(False)

    def run(*args, **kw):
        return _worker.submit(body, *args, **kw).result()

    sig = inspect.signature(fn)
    run.__signature__ = sig.replace(parameters=list(sig.parameters.values())[1:])
    run.__name__, run.__doc__, run.__module__ = fn.__name__, fn.__doc__, fn.__module__
    return run


def frame_streams():
    j, t, k = J(), T(), O.fixture_plain("compression_34k")
    return {"j4": (j * 4)[:3 * 65536 + 17], "jtk": j + t + k, "log": log_1m()}


def walk(f, cuts, sums):
    """the payloads of a frame without content size whose blocks hold `cuts` bytes: [(payload, stored raw?)]"""
    from lz4_flex_amd import frame
    assert f[:4] == (0x184D2204).to_bytes(4, "little")
    body, out = f[7:], []
    for _ in cuts:
        word = int.from_bytes(body[:4], "little")
        ln = word & 0x7FFFFFFF
        out.append((body[4:4 + ln], bool(word >> 31)))
        body = body[4 + ln + (4 if sums else 0):]
    assert body[:4] == bytes(4)                                       # the end mark
    return out


def stream_encode(frame, fi, data, piece):
    w = io.BytesIO()
    enc = frame.FrameEncoder.with_frame_info(fi, w)
    for at in range(0, len(data), piece):
        enc.write(data[at:at + piece])
    enc.finish()
    return w.getvalue()


def every_decoder(frame, f, data):
    from lz4_flex_amd import _lib
    lib = _lib.load()
    assert O.frame_decompress(f, len(data))[:2] == (0, data)
    assert O.c_frame_decompress(f, len(data)) == data
    assert frame.FrameDecoder.new(io.BytesIO(f)).read() == data
    assert frame.decompress_frames([f, f], len(data)) == [data, data]                # the chained path
    before = lib.lz4flex_get_tuning(None, b"decompress_level_chains")
    assert lib.lz4flex_set_tuning(None, b"decompress_level_chains", 1) == 0
    try:
        assert frame.decompress_frames([f, f], len(data)) == [data, data]            # the level path
    finally:
        assert lib.lz4flex_set_tuning(None, b"decompress_level_chains", before) == 0


TOTALS = {("log", 65536): (274737, 259660), ("log", 262144): (262691, 259588)}


@pytest.mark.parametrize("sums", [False, True], ids=["plain", "checksums"])
@pytest.mark.parametrize("bs", [4, 5], ids=["64K", "256K"])
@pytest.mark.parametrize("name", ["j4", "jtk", "log"])
@high_linked
def test_frames(block, name, bs, sums):
    from lz4_flex_amd import frame
    data = frame_streams()[name]
    cut = {4: 65536, 5: 262144}[bs]
    fi = frame.FrameInfo(block_size=frame.BlockSize(bs), block_mode=frame.BlockMode.Linked, block_checksums=sums, content_checksum=sums)
    one = frame.compress_frame(data, fi)
    # every block is the model's bytes, or raw where those are not smaller
    want = K.frame_payloads(data, cut, 16)
    assert walk(one, want, sums) == want
    if (name, cut) in TOTALS:
        ind, linked = TOTALS[(name, cut)]
        assert sum(len(p) for p, _ in K.frame_payloads(data, cut, 16, linked=False)) == ind
        assert sum(len(p) for p, _ in want) == linked
    # the three encoders agree
    pieces = (4093, 70001) + ((1,) if name == "j4" and bs == 4 and not sums else ())
    for piece in pieces:
        assert stream_encode(frame, fi, data, piece) == one, piece
    other = frame_streams()["jtk" if name != "jtk" else "j4"]
    many = frame.compress_frames([other[:70000], data, b"", data[:65537]], fi)
    assert many[1] == one and many[3] == frame.compress_frame(data[:65537], fi)
    every_decoder(frame, one, data)
    # smaller than mode 0's Linked frame and than mode 2's Independent frame
    ind = frame.compress_frame(data, frame.FrameInfo(block_size=frame.BlockSize(bs), block_mode=frame.BlockMode.Independent,
                                                     block_checksums=sums, content_checksum=sums))
    block.set_compress_mode("fast")
    try:
        fast = frame.compress_frame(data, fi)
    finally:
        block.set_compress_mode("high")
    print("%s, blocks of %d: high linked %d, fast linked %d, high independent %d" % (name, cut, len(one), len(fast), len(ind)))
    assert len(one) < len(fast)
    if len(want) > 1:
        assert len(one) < len(ind)
    else:       # (a stream of one block has no block with a history: the two frames carry the same payload)
        assert walk(ind, want, sums) == want


@high_linked
def test_a_flush_cuts_a_block_with_a_short_history(block):
    from lz4_flex_amd import frame
    data = frame_streams()["jtk"]
    fi = frame.FrameInfo(block_size=frame.BlockSize.Max64KB, block_mode=frame.BlockMode.Linked)
    w = io.BytesIO()
    enc = frame.FrameEncoder.with_frame_info(fi, w)
    enc.write(data[:100])
    enc.flush()
    enc.write(data[100:])
    enc.finish()
    f = w.getvalue()
    cuts = [(0, 100)] + [(at, min(65536, len(data) - at)) for at in range(100, len(data), 65536)]
    want = []
    for at, n in cuts:
        m = K.block(data, at, n, min(at, 32768), 16)
        want.append((m, False) if len(m) < n else (data[at:at + n], True))
    assert walk(f, want, False) == want
    assert want[1][0] == K.block(data, 100, 65536, 100, 16)
    assert O.frame_decompress(f, len(data))[:2] == (0, data)


@high_linked
def test_setting_0_a_linked_frame_is_mode_0s(block):
    from lz4_flex_amd import frame
    data = frame_streams()["j4"]
    fi = frame.FrameInfo(block_size=frame.BlockSize.Max64KB, block_mode=frame.BlockMode.Linked)
    on = frame.compress_frame(data, fi)
    block.set_compress_high_linked(False)
    off, off_many = frame.compress_frame(data, fi), frame.compress_frames([data, data[:70000]], fi)
    block.set_compress_mode("fast")
    try:
        assert off == frame.compress_frame(data, fi) and off_many == frame.compress_frames([data, data[:70000]], fi)
        # and mode 0 does not read the setting
        block.set_compress_high_linked(True)
        assert frame.compress_frame(data, fi) == off
    finally:
        block.set_compress_mode("high")
    assert on != off
    # Independent frames do not read it either
    fi = frame.FrameInfo(block_size=frame.BlockSize.Max64KB, block_mode=frame.BlockMode.Independent)
    on = frame.compress_frame(data, fi)
    block.set_compress_high_linked(False)
    assert frame.compress_frame(data, fi) == on


RULE_SETTINGS = ("compress_mode", "compress_high_linked", "compress_high_dict")


def rule_settings(lib):
    return {k: lib.lz4flex_get_tuning(None, k.encode()) for k in RULE_SETTINGS}


def frames_device(frame, streams, fi):
    """frame.compress_frames_device over streams that lie back to back in device memory: the frames"""
    import torch
    from lz4_flex_amd import _lib
    lib, dev = _lib.load(), torch.device("cuda", 0)
    in_len = [len(s) for s in streams]
    in_off = [sum(in_len[:i]) for i in range(len(streams))]
    cap = [int(lib.lz4flex_frame_compress_bound(n, C.byref(fi._c()))) for n in in_len]
    out_off = [sum(cap[:i]) for i in range(len(streams))]
    src = torch.from_numpy(np.frombuffer(b"".join(streams), dtype=np.uint8).copy()).to(dev)
    dst = torch.zeros(sum(cap), dtype=torch.uint8, device=dev)
    out_len, st = frame.compress_frames_device(src, in_off, in_len, fi, dst, out_off, cap)
    assert st == [0] * len(streams)
    host = dst.cpu().numpy()
    return [bytes(host[o:o + n]) for o, n in zip(out_off, out_len)]


@pytest.mark.parametrize("entry", ["streaming encoder", "compress_frames_device"])
@high_linked
def test_the_frame_layer_leaves_the_settings_alone(block, entry):
    """"compress_mode" 2 with "compress_high_linked" 0: a Linked frame is mode 0's, bytes for bytes, and the three settings the rule
    reads are what they were behind the call -- a successful one and one that "debug_fail_next_batch" made fail.  Two blocks of 64 KiB,
    the second with history; two streams side by side through the device entry."""
    from lz4_flex_amd import _lib, frame
    lib = _lib.load()
    data = frame_streams()["jtk"][:70000]
    fi = frame.FrameInfo(block_size=frame.BlockSize.Max64KB, block_mode=frame.BlockMode.Linked)

    def run():
        if entry == "streaming encoder":
            return [stream_encode(frame, fi, data, 70001)]
        return frames_device(frame, [data, data[1000:70000]], fi)

    on = run()                                         # (mode high, the setting on: the history form's frame)
    block.set_compress_high_linked(False)
    block.set_compress_mode("fast")
    fast = run()
    assert on != fast and all(O.frame_decompress(f, 70000)[:2] == (0, d) for f, d in zip(fast, (data, data[1000:70000])))
    block.set_compress_mode("high")
    want = {"compress_mode": 2, "compress_high_linked": 0, "compress_high_dict": 0}
    assert rule_settings(lib) == want
    assert run() == fast
    assert rule_settings(lib) == want
    assert lib.lz4flex_set_tuning(None, b"debug_fail_next_batch", 1) == 0
    with pytest.raises(frame.DeviceError, match="debug_fail_next_batch"):
        run()
    assert rule_settings(lib) == want
    assert run() == fast                               # (the hook is spent, the next call is an ordinary one)
    assert rule_settings(lib) == want


@high_linked
def test_packed_entry_follows_the_batch(block):
    """lz4flex_compress_batch_packed has no flag words: with the setting on its payloads are the batch's without flags, the plain model's"""
    j = J()
    blocks = [j[:5000], (j * 2)[100:100 + 70000], b"", j[40000:45000]]
    src = np.frombuffer(b"".join(blocks), dtype=np.uint8)
    in_len = np.array([len(b) for b in blocks], dtype=np.uint32)
    in_off = (np.cumsum(in_len.astype(np.uint64)) - in_len).astype(np.uint64)
    cap = np.array([O.max_out(len(b)) for b in blocks], dtype=np.uint32)
    slot = (np.cumsum(cap.astype(np.uint64)) - cap).astype(np.uint64)
    flat = np.zeros(int(cap.sum()), dtype=np.uint8)
    blen, st = block.compress_batch(src, in_off, in_len, flat, slot, cap)
    assert not st.any()
    out = np.zeros(sum(O.max_out(len(b)) + 4 for b in blocks), dtype=np.uint8)
    out_off, out_len, st = block.compress_batch_packed(src, in_off, in_len, out, prepend_size=False)
    assert not st.any()
    for k, b in enumerate(blocks):
        got = bytes(out[int(out_off[k]):int(out_off[k]) + int(out_len[k])])
        assert got == bytes(flat[int(slot[k]):int(slot[k]) + int(blen[k])]) == H.compress(b, 16), k
    # the same call with history flags: the model's bytes (block 3 has 75 000 bytes of the buffer in front of it)
    blen, st = block.compress_batch(src, in_off, in_len, flat, slot, cap, flags=[0, 5000 << 8, 0, 32768 << 8])
    assert not st.any()
    whole = bytes(src)
    for k, h in enumerate((0, 5000, 0, 32768)):
        assert bytes(flat[int(slot[k]):int(slot[k]) + int(blen[k])]) == K.block(whole, int(in_off[k]), len(blocks[k]), h, 16), k


@high_linked
def test_cli_high_linked(block, tmp_path):
    """--high --linked: the file is frame.compress_frame's Linked frame with the setting on, and the command line reads it back"""
    import os
    import subprocess
    import sys
    from lz4_flex_amd import frame
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data = frame_streams()["jtk"]
    src, dst, back = tmp_path / "in.bin", tmp_path / "in.bin.lz4", tmp_path / "back.bin"
    src.write_bytes(data)
    env = dict(os.environ, PYTHONPATH=root)
    env.pop("LZ4FLEX_HIGH_LINKED", None)
    subprocess.check_call([sys.executable, "-m", "lz4_flex_amd.cli", str(src), "-f", "-o", str(dst), "--high", "--linked"], env=env, cwd=root,
                          stdout=subprocess.DEVNULL)
    assert dst.read_bytes() == frame.compress_frame(data, frame.FrameInfo(block_mode=frame.BlockMode.Linked))
    subprocess.check_call([sys.executable, "-m", "lz4_flex_amd.cli", str(dst), "-f", "-o", str(back)], env=env, cwd=root, stdout=subprocess.DEVNULL)
    assert back.read_bytes() == data
