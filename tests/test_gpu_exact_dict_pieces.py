"""GPU: compress_mode 1 (reference-exact) calls with dictionaries, their chain records built in more than one piece.

A piece is as many blocks as the encoder workspace holds records for -- millions -- so only "debug_exact_dict_piece" makes a batch cross
a piece boundary.  Here a piece is 3 blocks and a batch 8: pieces [0, 3), [3, 6), [6, 8).  The blocks at 2 | 3 and 5 | 6 are unlike
neighbours (a refused block next to one without a dictionary), so an array indexed from the wrong end of a piece shows.  Every block's
bytes are the oracle's (compress_into_with_dict / compress) and those of the same call in one piece."""
import ctypes as C

import numpy as np
import pytest

import dict_cases as D
import oracle_api as O

pytestmark = pytest.mark.gpu

CANARY = 0xA5
PAD = 64
NONE = 0xFFFFFFFF
INVALID = 64
PIECE = 3
# dictionary + block of EDGE_DICT + 999 / + 1001 bytes: just below / above the 65 535 at which the reference changes its table kind
EDGE_DICT = 65535 - 1000
LONG = 70000                  # a dictionary of which the last 64 KiB are kept; a block the u16-table kernel must not take
SIZES = [300, 999, 700, 100, 1001, 2048, 1500, 1200]


def tail(kind, n):
    return D.dictionary(kind)[D.DICT_BYTES - n:] if n else b""


def blocks_of(sizes):
    return [D.block(("json", "text", "log")[j % 3], n, salt=j) for j, n in enumerate(sizes)]


def want_of(block, d):
    return O.compress_with_dict(block, d) if len(d) else O.compress(block)


@pytest.fixture(scope="module")
def env():
    import torch
    from lz4_flex_amd import _lib
    lib = _lib.load()
    assert lib.lz4flex_device_count() >= 1, _lib.last_error()
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
    assert lib.lz4flex_set_tuning(ctx, b"compress_mode", 1) == 0
    yield lib, _lib, torch, ctx
    lib.lz4flex_ctx_destroy(ctx)


class Arrays:
    """a call's arrays, host or device: p[name] is the pointer, fetch() the host copies behind the call"""

    def __init__(self, env, mem, **host):
        self.torch, self.mem, self.host = env[2], mem, {k: np.ascontiguousarray(v) for k, v in host.items()}
        if mem == "host":
            self.keep = self.host
            self.p = {k: C.c_void_p(v.ctypes.data) for k, v in self.host.items()}
        else:
            self.keep = {k: self.torch.from_numpy(v.view(np.uint8)).to("cuda") for k, v in self.host.items()}
            self.p = {k: C.c_void_p(v.data_ptr()) for k, v in self.keep.items()}

    def kind(self, L):
        return L.MEM_HOST if self.mem == "host" else L.MEM_DEVICE          # (never LZ4FLEX_MEM_BIG_BLOCKS)

    def stream(self):
        return None if self.mem == "host" else C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def fetch(self):
        if self.mem != "host":
            self.torch.cuda.synchronize()
            for k, v in self.keep.items():
                self.host[k].view(np.uint8)[:] = v.cpu().numpy()
        return self.host


def run(env, mem, blocks, piece, call, **extra):
    """one call on the batch `blocks` with pieces of `piece` blocks (0: one piece); call(lib, ctx, p, n, kind, stream) makes it.
    Returns (per block: the bytes produced, out_len, status, the slot as it is behind the call)."""
    lib, L, _, ctx = env
    n = len(blocks)
    in_off = np.cumsum([1] + [len(b) + 3 for b in blocks[:-1]]).astype(np.uint64)
    in_buf = np.full(int(in_off[-1]) + len(blocks[-1]) + PAD, CANARY, np.uint8)
    for o, b in zip(in_off, blocks):
        in_buf[int(o):int(o) + len(b)] = np.frombuffer(b, np.uint8)
    caps = np.array([O.max_out(len(b)) for b in blocks], np.uint32)
    out_off = np.cumsum([5] + [int(c) + PAD for c in caps[:-1]]).astype(np.uint64)
    out = np.full(int(out_off[-1]) + int(caps[-1]) + PAD, CANARY, np.uint8)
    a = Arrays(env, mem, in_buf=in_buf, in_off=in_off, in_len=np.array([len(b) for b in blocks], np.uint32), out=out, out_off=out_off,
               out_cap=caps, out_len=np.full(n, 0xDEAD, np.uint32), status=np.full(n, -1, np.int32), **extra)
    assert lib.lz4flex_set_tuning(ctx, b"debug_exact_dict_piece", piece) == 0
    try:
        rc = call(lib, ctx, a.p, n, a.kind(L), a.stream())
        h = a.fetch()
    finally:
        assert lib.lz4flex_set_tuning(ctx, b"debug_exact_dict_piece", 0) == 0
    assert rc == 0, (rc, L.last_error())
    assert np.array_equal(h["in_buf"], in_buf), "the input was written"
    slots = [h["out"][int(o):int(o) + int(c)] for o, c in zip(out_off, caps)]
    between = np.ones(len(out), bool)
    for o, c in zip(out_off, caps):
        between[int(o):int(o) + int(c)] = False
    assert (h["out"][between] == CANARY).all(), "bytes outside the output slots were written"
    return [bytes(s[:int(m)]) for s, m in zip(slots, h["out_len"])], h["out_len"].copy(), h["status"].copy(), slots


def check(env, mem, blocks, dicts_of_blocks, refused, long_blocks, call, **extra):
    """dicts_of_blocks[i]: block i's dictionary (b"": none); refused / long_blocks: the indices that come back INVALID_ARG"""
    n = len(blocks)
    assert n == 8 and -(-n // PIECE) == 3
    got, one = run(env, mem, blocks, PIECE, call, **extra), run(env, mem, blocks, 0, call, **extra)
    bad = set(refused) | set(long_blocks)
    for i in range(n):
        print(i, len(blocks[i]), len(dicts_of_blocks[i]), int(got[2][i]), int(got[1][i]))
        assert int(got[2][i]) == (INVALID if i in bad else 0), i
        assert int(one[2][i]) == int(got[2][i]) and int(one[1][i]) == int(got[1][i]), i
        if i in bad:
            assert int(got[1][i]) == 0, i
        else:
            assert got[0][i] == want_of(blocks[i], dicts_of_blocks[i]), (i, len(blocks[i]), len(dicts_of_blocks[i]))
            assert got[0][i] == one[0][i], i
        if i in refused:
            assert (got[3][i] == CANARY).all() and (one[3][i] == CANARY).all(), "the slot of refused block %d was written" % i


def sizes_for(mem):
    """DEVICE memory, no LZ4FLEX_MEM_BIG_BLOCKS: block 5 (without a dictionary) breaks the promise of blocks of at most 64 KiB"""
    return [LONG if (mem == "device" and i == 5) else s for i, s in enumerate(SIZES)]


@pytest.mark.parametrize("mem", ["host", "device"])
def test_batch_ex(env, mem):
    blocks = blocks_of(sizes_for(mem))
    ds = [tail("json", 1), tail("text", EDGE_DICT), tail("log", 500), b"", tail("text", EDGE_DICT), b"", tail("json", 500), tail("log", LONG)]
    refused = [2, 6]
    doff = np.cumsum([7] + [len(d) + 1 for d in ds[:-1]]).astype(np.uint64)
    dbuf = np.full(int(doff[-1]) + len(ds[-1]) + PAD, CANARY, np.uint8)
    for o, d in zip(doff, ds):
        dbuf[int(o):int(o) + len(d)] = np.frombuffer(d, np.uint8)
    flags = np.array([1 if i in refused else 0 for i in range(8)], np.uint32)

    def call(lib, ctx, p, n, kind, stream):
        e = env[1].CompressExt(p["dbuf"], p["doff"], p["dlen"])
        return lib.lz4flex_compress_batch_ex(ctx, p["in_buf"], p["in_off"], p["in_len"], p["flags"], n, p["out"], p["out_off"], p["out_cap"],
                                             p["out_len"], p["status"], C.byref(e), kind, stream)

    check(env, mem, blocks, ds, refused, [5] if mem == "device" else [], call, dbuf=dbuf, doff=doff,
          dlen=np.array([len(d) for d in ds], np.uint32), flags=flags)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("dict_len", [1, EDGE_DICT, LONG])
def test_shared_dict(env, dict_len, mem):
    """every block has the one dictionary: no block without one, none refused"""
    blocks = blocks_of(SIZES)
    d = tail("text", dict_len)

    def call(lib, ctx, p, n, kind, stream):
        return lib.lz4flex_compress_batch_shared_dict(ctx, p["in_buf"], p["in_off"], p["in_len"], n, p["out"], p["out_off"], p["out_cap"],
                                                      p["out_len"], p["status"], p["dict"], len(d), kind, stream)

    check(env, mem, blocks, [d] * 8, [], [], call, dict=np.frombuffer(d, np.uint8).copy())


@pytest.mark.parametrize("mem", ["host", "device"])
def test_dict_set(env, mem):
    lib, L, torch, ctx = env
    recs = [tail("json", 1), tail("text", EDGE_DICT), tail("log", LONG), b""]         # (record 3: a dictionary of length 0 is none)
    k = len(recs)
    ids = [0, 1, k, 3, 1, NONE, k, 2]
    blocks = blocks_of(sizes_for(mem))
    roff = np.cumsum([3] + [len(r) + 5 for r in recs[:-1]]).astype(np.uint64)
    rbuf = np.full(int(roff[-1]) + PAD, CANARY, np.uint8)
    for o, r in zip(roff, recs):
        rbuf[int(o):int(o) + len(r)] = np.frombuffer(r, np.uint8)
    rlen = np.array([len(r) for r in recs], np.uint32)
    h = C.c_void_p()
    assert lib.lz4flex_dict_set_create(ctx, C.c_void_p(rbuf.ctypes.data), C.c_void_p(roff.ctypes.data), C.c_void_p(rlen.ctypes.data), k,
                                       L.MEM_HOST, C.byref(h)) == 0 and h.value, L.last_error()

    def call(lib, ctx, p, n, kind, stream):
        return lib.lz4flex_compress_batch_dict_set(ctx, p["in_buf"], p["in_off"], p["in_len"], n, p["ids"], p["out"], p["out_off"], p["out_cap"],
                                                   p["out_len"], p["status"], h, kind, stream)

    try:
        check(env, mem, blocks, [recs[i] if i < k else b"" for i in ids], [2, 6], [5] if mem == "device" else [], call,
              ids=np.array(ids, np.uint32))
    finally:
        torch.cuda.synchronize()
        lib.lz4flex_dict_set_free(h)
