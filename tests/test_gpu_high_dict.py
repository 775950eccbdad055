"""GPU (-m gpu): compress_mode 2 ("high") against dictionaries ("compress_high_dict" 1; lz4_compress_high.hip, the dictionary form)
through the C ABI.  The kernel must reproduce the scalar definition (tests/sim/high_dict_model.c) byte for byte, through every entry
that takes dictionaries, in host and in device memory, with the shared dictionary's digest and without it; with the setting at 0, and
in the other modes, nothing changes."""
import ctypes as C
import random

import numpy as np
import pytest

import hc_dict_model as D
import oracle_api as O

pytestmark = pytest.mark.gpu

CANARY = 16
NO_DICT = 0xFFFFFFFF
BLOCK_LENS = (0, 1, 11, 12, 13, 17, 4095, 4096, 32767, 32768, 32769, 32780, 65536, 65537, 98305)
DICT_LENS = (0, 3, 4, 5, 7, 15, 1027, 4096, 32767, 32768, 32769, 65536, 70000)
KINDS = ("json", "text", "zeros", "period256", "ab", "pieces")


def pair(kind, dl, n, rnd):
    """(dictionary of dl bytes, block of n bytes) of one kind"""
    if kind in ("json", "text"):
        s = O.fixture_plain("compression_66k_JSON" if kind == "json" else "compression_65k") * 4
        at = rnd.randrange(0, 2000)
        return s[at:at + dl], s[at + dl:at + dl + n]
    if kind == "zeros":
        return bytes(dl), bytes(n)
    if kind == "period256":
        s = bytes(range(256)) * ((dl + n) // 256 + 2)
        return s[5:5 + dl], s[5 + dl:5 + dl + n]
    if kind == "ab":
        s = bytes(rnd.choice(b"ab") for _ in range(dl + n))
        return s[:dl], s[dl:]
    d = bytes(rnd.getrandbits(8) for _ in range(dl))            # pieces of a random dictionary between random bytes
    out = bytearray()
    while len(out) < n:
        if dl >= 8 and rnd.random() < 0.7:
            ln = rnd.randint(4, min(300, dl))
            at = rnd.randrange(0, dl - ln + 1) if rnd.random() < 0.5 else dl - ln - rnd.randrange(0, min(64, dl - ln + 1))
            out += d[at:at + ln]
        else:
            out += bytes(rnd.getrandbits(8) for _ in range(rnd.randint(1, 40)))
    return d, bytes(out[:n])


_batch = []


def batch():
    """every block length with four dictionary lengths, the lengths and the contents in rotation: 60 (dictionary, block) pairs"""
    if not _batch:
        rnd = random.Random(1717)
        for i, n in enumerate(BLOCK_LENS):
            for k in range(4):
                _batch.append(pair(KINDS[(i + k) % 6], DICT_LENS[(4 * i + k) % 13], n, rnd))
    return _batch


_model = {}


def model(data, d, depth):
    d = d[-32768:] if len(d) >= 4 else b""                       # (what the definition reads of it)
    key = (data, d, depth)
    if key not in _model:
        _model[key] = D.compress(data, d, depth)
    return _model[key]


@pytest.fixture(scope="module")
def env():
    from lz4_flex_amd import _lib
    lib = _lib.load()
    assert lib.lz4flex_device_count() >= 1
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
    for key, v in ((b"compress_mode", 2), (b"compress_high_dict", 1), (b"compress_depth", 16)):
        assert lib.lz4flex_set_tuning(ctx, key, v) == 0
    yield lib, ctx
    lib.lz4flex_ctx_destroy(ctx)


def tune(env, **kv):
    lib, ctx = env
    for key, v in kv.items():
        assert lib.lz4flex_set_tuning(ctx, key.encode(), v) == 0, key


class Mem:
    """the arrays of one call in host or in device memory"""

    def __init__(self, device):
        self.device, self.keep = device, []

    def put(self, a):
        if a is None:
            return None
        if not self.device:
            self.keep.append(a)
            return C.c_void_p(a.ctypes.data)
        import torch
        dt = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype)
        t = torch.from_numpy((a if a.flags.writeable else a.copy()).view(dt)).to(torch.device("cuda", 0))
        self.keep.append(t)
        return C.c_void_p(t.data_ptr())

    def get(self, i, like):
        if not self.device:
            return self.keep[i]
        import torch
        torch.cuda.synchronize()
        return self.keep[i].cpu().numpy().view(like.dtype)


def pack(parts, pad):
    """the parts one after the other with `pad` bytes between them: (buffer, offsets, lengths)"""
    ln = np.array([len(p) for p in parts], dtype=np.uint32)
    off = np.zeros(len(parts), dtype=np.uint64)
    off[1:] = np.cumsum(ln.astype(np.uint64) + pad)[:-1]
    buf = np.zeros(int(off[-1] + ln[-1]) + 64, dtype=np.uint8)
    for p, o in zip(parts, off):
        buf[int(o):int(o) + len(p)] = np.frombuffer(p, dtype=np.uint8)
    return buf, off, ln


def encode(env, entry, device, blocks, dicts=None, shared=None, ids=None, dset=None, caps=None, flags=None, in_shift=0, shared_shift=0):
    """one call of lz4flex_compress_batch_<entry> ("ex", "shared_dict", "dict_set"): unaligned block starts, output slots of `caps`
    (default: the bound) with CANARY bytes of 0xEE in front of and behind each.  Returns (the whole output buffer, out_off, out_len, status)."""
    from lz4_flex_amd import _lib as L
    lib, ctx = env
    n = len(blocks)
    buf, in_off, in_len = pack(blocks, 3)
    if in_shift:
        buf, in_off = np.concatenate([np.zeros(in_shift, dtype=np.uint8), buf]), in_off + np.uint64(in_shift)
    cap = np.array([O.max_out(len(b)) for b in blocks] if caps is None else caps, dtype=np.uint32)
    out_off = (np.cumsum(cap.astype(np.uint64) + CANARY) - cap).astype(np.uint64)
    out = np.full(int(out_off[-1] + cap[-1]) + CANARY, 0xEE, dtype=np.uint8)
    out_len, st = np.zeros(n, dtype=np.uint32), np.full(n, -1, dtype=np.int32)
    m = Mem(device)
    p_out, p_len, p_st = m.put(out), m.put(out_len), m.put(st)
    head = [m.put(buf), m.put(in_off), m.put(in_len)]
    slots = [p_out, m.put(out_off), m.put(cap), p_len, p_st]
    mem = L.MEM_DEVICE if device else L.MEM_HOST
    if entry == "ex":
        dbuf, d_off, d_len = pack(dicts, 1)
        ext = L.CompressExt(m.put(dbuf).value, m.put(d_off).value, m.put(d_len).value)
        fl = None if flags is None else m.put(np.array(flags, dtype=np.uint32))
        rc = lib.lz4flex_compress_batch_ex(ctx, *head, fl, n, *slots, C.byref(ext), mem, None)
    elif entry == "shared_dict":
        dbuf = np.frombuffer(bytes(shared_shift) + shared + b"\0", dtype=np.uint8)
        at = C.c_void_p(m.put(dbuf).value + shared_shift)
        rc = lib.lz4flex_compress_batch_shared_dict(ctx, *head, n, *slots, at, len(shared), mem, None)
    else:
        rc = lib.lz4flex_compress_batch_dict_set(ctx, *head, n, m.put(np.array(ids, dtype=np.uint32)), *slots, dset.handle, mem, None)
    assert rc == 0, L.last_error()
    return m.get(0, out), out_off, m.get(1, out_len), m.get(2, st)


def check(blocks, dicts, depth, res, refused=None):
    """every slot holds the model's bytes (a refused one: its status and nothing) and every byte outside the blocks' bytes is untouched"""
    out, out_off, out_len, st = res
    refused = refused or {}
    want = np.full(out.size, 0xEE, dtype=np.uint8)
    for k, b in enumerate(blocks):
        if k in refused:
            assert (int(st[k]), int(out_len[k])) == (refused[k], 0), k
            continue
        m = model(b, dicts[k], depth)
        assert int(st[k]) == 0 and int(out_len[k]) == len(m), (k, len(b), len(dicts[k]), int(st[k]), int(out_len[k]), len(m))
        want[int(out_off[k]):int(out_off[k]) + len(m)] = np.frombuffer(m, dtype=np.uint8)
    bad = np.flatnonzero(want != out)
    if bad.size:
        k = int(np.searchsorted(out_off, bad[0], side="right")) - 1
        raise AssertionError("first difference at output byte %d: block %d (length %d, dictionary %d), byte %d of its slot"
                             % (bad[0], k, len(blocks[k]), len(dicts[k]), bad[0] - int(out_off[k])))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("depth", [1, 16])
def test_ex_equals_model(env, depth, device):
    tune(env, compress_depth=depth)
    dicts, blocks = zip(*batch())
    check(blocks, dicts, depth, encode(env, "ex", device, blocks, dicts=dicts))


def test_ex_equals_model_depth_64(env):
    tune(env, compress_depth=64)
    try:
        dicts, blocks = zip(*batch())
        check(blocks, dicts, 64, encode(env, "ex", True, blocks, dicts=dicts))
    finally:
        tune(env, compress_depth=16)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("depth", [1, 16])
def test_dict_set_equals_model(env, depth, device):
    from lz4_flex_amd import _lib as L, block
    tune(env, compress_depth=depth)
    dicts, blocks = zip(*batch())
    k = len(dicts)
    # ids 0, 1, ..., then a block without a dictionary and one whose id the set does not have
    blocks = list(blocks) + [blocks[25], blocks[26]]
    seen = list(dicts) + [b"", b""]
    ids = list(range(k)) + [NO_DICT, k]
    with block.DictSet(list(dicts), ctx=env[1]) as ds:
        res = encode(env, "dict_set", device, blocks, ids=ids, dset=ds)
    check(blocks, seen, depth, res, refused={k + 1: L.E_INVALID_ARG})


@pytest.mark.parametrize("digest", [1, 0])
@pytest.mark.parametrize("depth", [1, 16])
def test_shared_dict_equals_model(env, depth, digest):
    tune(env, compress_depth=depth, compress_high_digest=digest)
    try:
        rnd = random.Random(99)
        for i, dl in enumerate(DICT_LENS):
            d, long = pair(KINDS[i % 6], dl, 98305, rnd)
            blocks = [long[:n] for n in BLOCK_LENS]
            check(blocks, [d] * len(blocks), depth, encode(env, "shared_dict", bool(i & 1), blocks, shared=d))
    finally:
        tune(env, compress_high_digest=1)


@pytest.mark.parametrize("dl", [4096, 32768])
def test_every_alignment(env, dl):
    """(block address, dictionary end) mod 4: all 16 through _ex, and through the shared entry with its digest"""
    tune(env, compress_depth=16)
    j = O.fixture_plain("compression_66k_JSON")
    blocks = [j[40000 + k:44096 + k] for k in range(4)]
    dicts = [j[k:k + dl] for k in range(4)]
    # device allocations are aligned: pack() puts block k at 4099 k + shift and ends dictionary k at (dl + 1) k + dl, so the
    # residues are (3 k + shift, k) -- every pair over the four shifts
    for shift in range(4):
        check(blocks, dicts, 16, encode(env, "ex", True, blocks, dicts=dicts, in_shift=shift))
    # the shared entry: the blocks at the residues 0, 3, 2, 1, the dictionary's end at each of the four
    for shift in range(4):
        check(blocks, [dicts[0]] * 4, 16, encode(env, "shared_dict", True, blocks, shared=dicts[0], shared_shift=shift))


def log_records(lib):
    from lz4_flex_amd import workloads
    n = 2 * lib.lz4flex_get_tuning(None, b"compress_workgroups") + 3
    rnd = random.Random(7)
    log = bytes(workloads.log_stream(0, 1 << 20).numpy())
    out = []
    for _ in range(n):
        ln = rnd.randint(1024, 3072)
        at = rnd.randrange(40000, len(log) - ln)
        out.append(log[at:at + ln])
    return log[:32768], out


@pytest.mark.parametrize("digest", [1, 0])
def test_more_blocks_than_workgroups(env, digest):
    from lz4_flex_amd import _lib as L
    tune(env, compress_depth=16, compress_high_digest=digest)
    try:
        d, blocks = log_records(env[0])
        refused = {k: L.E_OUTPUT_TOO_SMALL for k in range(6, len(blocks), 7)}
        caps = [O.max_out(len(b)) - (1 if k in refused else 0) for k, b in enumerate(blocks)]
        check(blocks, [d] * len(blocks), 16, encode(env, "shared_dict", True, blocks, shared=d, caps=caps), refused)
    finally:
        tune(env, compress_high_digest=1)


def test_mixed_batch_keeps_no_state(env):
    """a dictionary, none, one of 3 bytes, in turn: more blocks than a workgroup's first, so every workgroup meets all three"""
    tune(env, compress_depth=16)
    j = O.fixture_plain("compression_66k_JSON") * 3
    n = 3 * (env[0].lz4flex_get_tuning(None, b"compress_workgroups") // 2) + 5
    rnd = random.Random(3)
    blocks, dicts = [], []
    for k in range(n):
        ln = 70000 if k % 50 == 7 else rnd.randint(100, 3000)
        at = rnd.randrange(33000, 60000)
        blocks.append(j[at:at + ln])
        dicts.append((j[at - 32768:at] if k % 6 else j[:5000], b"", j[:3])[k % 3])
    check(blocks, dicts, 16, encode(env, "ex", True, blocks, dicts=dicts))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_ex_refuses_a_dictionary_with_flags(env, device):
    from lz4_flex_amd import _lib as L
    tune(env, compress_depth=16)
    j = O.fixture_plain("compression_66k_JSON")
    blocks = [j[40000:44096], j[40000:44096], j[50000:50100], j[41000:45000]]
    dicts = [j[:32768], j[:32768], b"", j[:4096]]
    # blocks 1 and 3: a dictionary and a flag word -- refused; block 2 has no dictionary: its flags are not read in this mode
    # (in_shift: a host batch wants the 32 KiB its history bits speak of to lie inside the buffer)
    res = encode(env, "ex", device, blocks, dicts=dicts, flags=[0, 32768 << 8, 32768 << 8, 1], in_shift=40000)
    check(blocks, dicts, 16, res, refused={1: L.E_INVALID_ARG, 3: L.E_INVALID_ARG})


@pytest.fixture
def high_default():
    """this thread's default context in mode high with the dictionary form; fast again afterwards"""
    from lz4_flex_amd import block
    block.set_compress_mode("high")
    block.set_compress_depth(16)
    block.set_compress_high_dict(True)
    yield block
    block.set_compress_mode("fast")
    block.set_compress_high_dict(False)


def test_scalar_entries(high_default):
    block = high_default
    j = O.fixture_plain("compression_66k_JSON")
    for data, d in ((j[40000:44096], j[:32768]), (j[41000:], j[:40000]), (j[50000:50100], j[:4096]), (b"", j[:100]), ((j * 3)[:150000], j[100:30000])):
        assert block.compress_with_dict(data, d) == model(data, d, 16)
        assert block.compress_prepend_size_with_dict(data, d) == len(data).to_bytes(4, "little") + model(data, d, 16)


def shared_call(block, blocks, d):
    src = np.frombuffer(b"".join(blocks), dtype=np.uint8)
    in_len = np.array([len(b) for b in blocks], dtype=np.uint32)
    in_off = (np.cumsum(in_len.astype(np.uint64)) - in_len).astype(np.uint64)
    cap = np.array([O.max_out(len(b)) for b in blocks], dtype=np.uint32)
    out_off = (np.cumsum(cap.astype(np.uint64)) - cap).astype(np.uint64)
    out = np.zeros(int(cap.sum()), dtype=np.uint8)
    out_len, st = block.compress_batch_with_shared_dict(src, in_off, in_len, np.frombuffer(d, dtype=np.uint8), out, out_off, cap)
    assert not st.any()
    return [bytes(out[int(o):int(o) + int(n)]) for o, n in zip(out_off, out_len)]


def test_the_setting(high_default):
    block = high_default
    j = O.fixture_plain("compression_66k_JSON")
    blocks, d = [j[40000:44096], j[50000:50100], (j * 2)[41000:120000]], j[:32768]
    want = [model(b, d, 16) for b in blocks]
    assert shared_call(block, blocks, d) == want
    got = {}
    for mode in ("fast", "exact"):
        block.set_compress_mode(mode)
        try:
            got[mode] = shared_call(block, blocks, d)
            block.set_compress_high_dict(False)
            assert shared_call(block, blocks, d) == got[mode]      # the setting is not read in these modes
        finally:
            block.set_compress_high_dict(True)
            block.set_compress_mode("high")
    assert got["fast"] != want and got["exact"] != want
    block.set_compress_high_dict(False)                           # off again in the same context: mode 0's bytes
    try:
        assert shared_call(block, blocks, d) == got["fast"]
    finally:
        block.set_compress_high_dict(True)
    assert shared_call(block, blocks, d) == want


def test_every_dictionary_decoder_reads_the_blocks(high_default):
    block = high_default
    j = O.fixture_plain("compression_66k_JSON") * 3
    d = j[:32768]
    blocks = [j[40000:44096], j[50000:50100], j[41000:120000], j[40000:40013], b"", j[33000:98536]]
    comp = shared_call(block, blocks, d)
    assert comp == [model(b, d, 16) for b in blocks]
    n = len(blocks)
    src = np.frombuffer(b"".join(comp), dtype=np.uint8)
    in_len = np.array([len(c) for c in comp], dtype=np.uint32)
    in_off = (np.cumsum(in_len.astype(np.uint64)) - in_len).astype(np.uint64)
    cap = np.array([len(b) for b in blocks], dtype=np.uint32)
    out_off = (np.cumsum(cap.astype(np.uint64)) - cap).astype(np.uint64)
    plain = np.frombuffer(b"".join(blocks), dtype=np.uint8)
    dn = np.frombuffer(d, dtype=np.uint8)

    def whole(res, out):
        assert not res[1].any() and res[0].tolist() == cap.tolist()
        assert np.array_equal(out[:-1], plain)

    out = np.zeros(plain.size + 1, dtype=np.uint8)
    whole(block.decompress_batch_with_shared_dict(src, in_off, in_len, dn, out, out_off, cap), out)
    out = np.zeros(plain.size + 1, dtype=np.uint8)
    whole(block.decompress_batch_with_dict(src, in_off, in_len, dn, np.zeros(n, dtype=np.uint64), np.full(n, len(d), dtype=np.uint32), out, out_off, cap), out)
    with block.DictSet([b"xyz", dn]) as ds:
        out = np.zeros(plain.size + 1, dtype=np.uint8)
        whole(block.decompress_batch_with_dict_set(src, in_off, in_len, [1] * n, ds, out, out_off, cap), out)
    out = np.zeros(plain.size + 1, dtype=np.uint8)
    whole(block.decompress_batch_partial_with_shared_dict(src, in_off, in_len, dn, out, out_off, cap), out)
    tgt = np.minimum(cap, 64).astype(np.uint32)
    t_off = (np.cumsum(tgt.astype(np.uint64)) - tgt).astype(np.uint64)
    out = np.zeros(int(tgt.sum()) + 1, dtype=np.uint8)
    out_len, st = block.decompress_batch_partial_with_shared_dict(src, in_off, in_len, dn, out, t_off, np.full(n, 64, dtype=np.uint32))
    assert not st.any() and out_len.tolist() == tgt.tolist()
    assert bytes(out[:-1]) == b"".join(b[:64] for b in blocks)
