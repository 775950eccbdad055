"""GPU (-m gpu): what every batched entry point of the C ABI shares (capi.cpp) -- the mem_kind values each one accepts, and the event
that orders a context's shared workspaces (the throughput encoder's, the chained decoder's "done" words, the paired workgroup decoder's
hand-over area) between batches on different streams."""
import ctypes as C

import numpy as np
import pytest

import dict_cases as D
import oracle_api as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from lz4_flex_amd import _lib
    lib = _lib.load()
    assert lib.lz4flex_device_count() >= 1, _lib.last_error()
    return lib, _lib, torch


def _ctx(lib, **tuning):
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
    for k, v in tuning.items():
        assert lib.lz4flex_set_tuning(ctx, k.encode(), v) == 0, k
    return ctx


class Arrays:
    """named numpy arrays in host memory or copied to the device; ptr(name) for the call, fetch() brings them back"""

    def __init__(self, torch, device, **arrays):
        self.torch, self.device, self.host = torch, device, arrays
        if device:
            self.dev = {k: torch.from_numpy(v.view(np.uint8).reshape(-1)).to("cuda:0") for k, v in arrays.items()}
            torch.cuda.synchronize()

    def ptr(self, name, at=0):
        return C.c_void_p((self.dev[name].data_ptr() if self.device else self.host[name].ctypes.data) + at)

    def fetch(self):
        if self.device:
            self.torch.cuda.synchronize()
            return {k: v.cpu().numpy().view(self.host[k].dtype).reshape(self.host[k].shape) for k, v in self.dev.items()}
        return self.host


# ---------------------------------------------------------------- mem_kind
KINDS = [0, 1, 0x100, 0x101, 0x200, 0x201, 0x301, 7, 0x1000, 0x1001]
PLAIN = b"sixteen bytes..!"
BLOCK = bytes([0x10, 0x61, 0x01, 0x00, 0xB0]) + b"eleven bytes"[:11]       # 'a', a match of 4 at offset 1, 11 literals: 16 bytes -> 16 bytes
DICT = b"a dictionary of some bytes, 40 of them.."
assert len(PLAIN) == 16 and len(BLOCK) == 16

# entry -> (mem_kind values accepted in host memory, in device memory)
LOW0, LOW1 = {0, 0x100, 0x200, 0x1000}, {1, 0x101, 0x201, 0x301, 0x1001}
ACCEPTS = {
    "compress_batch": ({0}, LOW1),
    "compress_batch_ex": ({0}, {1, 0x101}),
    "compress_batch_shared_dict": ({0}, {1, 0x101}),
    # lz4flex_decompress_batch accepts every mem_kind lz4flex_decompress_batch_ex does, but it has no way to hand over the out_pos a CHAINED
    # batch needs: the chained kinds get past the mem_kind check and are refused as a chain without positions -- the same answer
    "decompress_batch": (LOW0 - {0x200}, LOW1 - {0x201, 0x301}),
    "decompress_batch_ex": (LOW0, LOW1),
    "decompress_batch_shared_dict": ({0, 0x100}, {1, 0x101}),
    "decompressed_size_batch": ({0, 0x100}, {1, 0x101}),
}


@pytest.mark.parametrize("entry", sorted(ACCEPTS))
def test_mem_kind_sweep(env, entry):
    lib, L, torch = env
    assert O.decompress(BLOCK, 16)[0] == "ok"
    compress = entry.startswith("compress")
    ctx = _ctx(lib)
    try:
        for mem in KINDS:
            host_ok, dev_ok = ACCEPTS[entry]
            device = (mem & 0xFF) == L.MEM_DEVICE
            a = Arrays(torch, device, src=np.frombuffer(PLAIN if compress else BLOCK, dtype=np.uint8).copy(), in_off=np.zeros(1, np.uint64),
                       in_len=np.full(1, 16, np.uint32), sink=np.full(64, 0xA5, np.uint8), out_off=np.zeros(1, np.uint64),
                       cap=np.full(1, 64, np.uint32), out_len=np.full(1, 0xDEADBEEF, np.uint32), status=np.full(1, -1, np.int32),
                       detail=np.full(2, 0xEE, np.uint64), size=np.full(1, 0xEEEE, np.uint64), dic=np.frombuffer(DICT, dtype=np.uint8).copy(),
                       dict_len=np.full(1, len(DICT), np.uint32), pos=np.zeros(1, np.uint32))
            p = a.ptr
            head = (ctx, p("src"), p("in_off"), p("in_len"))
            outs = (p("sink"), p("out_off"), p("cap"), p("out_len"), p("status"))
            if entry == "compress_batch":
                rc = lib.lz4flex_compress_batch(*head, None, 1, *outs, mem, None)
            elif entry == "compress_batch_ex":
                ext = L.CompressExt(p("dic"), p("in_off"), p("dict_len"))
                rc = lib.lz4flex_compress_batch_ex(*head, None, 1, *outs, C.byref(ext), mem, None)
            elif entry == "compress_batch_shared_dict":
                rc = lib.lz4flex_compress_batch_shared_dict(*head, 1, *outs, p("dic"), len(DICT), mem, None)
            elif entry == "decompress_batch":
                rc = lib.lz4flex_decompress_batch(*head, 1, *outs, p("detail"), mem, None)
            elif entry == "decompress_batch_ex":
                ext = L.DecompressExt(None, None, None, p("pos"), None, 0)      # a valid out_pos: acceptance is about mem_kind alone
                rc = lib.lz4flex_decompress_batch_ex(*head, 1, *outs, p("detail"), C.byref(ext), mem, None)
            elif entry == "decompress_batch_shared_dict":
                rc = lib.lz4flex_decompress_batch_shared_dict(*head, 1, *outs, p("detail"), p("dic"), len(DICT), mem, None)
            else:
                rc = lib.lz4flex_decompressed_size_batch(*head, 1, None, p("size"), p("status"), mem, None)
            got = a.fetch()
            what = (entry, hex(mem))
            if mem in (dev_ok if device else host_ok):
                assert rc == 0, (what, rc, L.last_error())
                assert int(got["status"][0]) == 0, (what, got["status"])
                if entry == "decompressed_size_batch":
                    assert int(got["size"][0]) == 16, what
                elif compress:
                    n = int(got["out_len"][0])
                    assert 0 < n <= 64, what
                    assert O.decompress(got["sink"][:n].tobytes(), 16, dict_data=DICT if "dict" in entry or "ex" in entry else None) == ("ok", PLAIN), what
                else:
                    assert int(got["out_len"][0]) == 16 and got["sink"][:16].tobytes() == O.decompress(BLOCK, 16)[1], what
            else:
                assert rc == -L.E_INVALID_ARG, (what, rc)
                assert int(got["status"][0]) == -1 and int(got["out_len"][0]) == 0xDEADBEEF and int(got["size"][0]) == 0xEEEE, what
                assert bool((got["sink"] == 0xA5).all()), what
    finally:
        lib.lz4flex_ctx_destroy(ctx)


# ---------------------------------------------------------------- one workspace, two streams
def _encode_job(which):
    """8 blocks of 4 KiB for the throughput encoder (its persistent workgroups' workspace)"""
    plain = b"".join(D.block(("text", "json")[which], 4096, 10 * which + i) for i in range(8))
    cap = O.max_out(4096)
    return dict(compress=True, src=plain, in_off=[4096 * i for i in range(8)], in_len=[4096] * 8, out_off=[cap * i for i in range(8)], cap=[cap] * 8,
                out_bytes=cap * 8, pos=None, flags=0)


def _chain_job(which):
    """4 blocks of 1 KiB in one chain: every block is encoded with everything before it as its dictionary, so it decodes behind those bytes only"""
    plain = D.block(("log", "text")[which], 4096, 40 + which)
    comps = [O.compress_with_dict(plain[1024 * i:1024 * (i + 1)], plain[:1024 * i]) if i else O.compress(plain[:1024]) for i in range(4)]
    lens = [len(c) for c in comps]
    return dict(compress=False, src=b"".join(comps), in_off=[sum(lens[:i]) for i in range(4)], in_len=lens, out_off=[0] * 4, cap=[4096] * 4,
                out_bytes=4096, pos=[1024 * i for i in range(4)], flags="chained", plain=plain)


def _pair_job(which):
    """2 blocks of 8 KiB for the workgroup decoder with a parser and a copier workgroup per block ("decompress_pcd_pair" 2)"""
    plains = [D.block(("json", "log")[which], 8192, 70 + 2 * which + i) for i in range(2)]
    comps = [O.compress(p) for p in plains]
    lens = [len(c) for c in comps]
    return dict(compress=False, src=b"".join(comps), in_off=[0, lens[0]], in_len=lens, out_off=[0, 8192], cap=[8192] * 2, out_bytes=16384, pos=None,
                flags=0, plain=b"".join(plains))


def _stage(env, job):
    """the job's arrays in device memory (waits for the copies)"""
    lib, L, torch = env
    n = len(job["in_len"])
    return Arrays(torch, True, src=np.frombuffer(job["src"] + bytes(64), dtype=np.uint8).copy(), in_off=np.array(job["in_off"], np.uint64),
                  in_len=np.array(job["in_len"], np.uint32), sink=np.full(job["out_bytes"] + 64, 0xA5, np.uint8), out_off=np.array(job["out_off"], np.uint64),
                  cap=np.array(job["cap"], np.uint32), out_len=np.full(n, 0xDEADBEEF, np.uint32), status=np.full(n, -1, np.int32),
                  pos=np.array(job["pos"] or [0] * n, np.uint32))


def _issue(env, ctx, job, a, stream):
    """enqueue the job as a MEM_DEVICE batch on `stream`, on the staged arrays `a`: the C call and nothing else touches the device"""
    lib, L, torch = env
    n = len(job["in_len"])
    p = a.ptr
    mem = L.MEM_DEVICE | (L.MEM_CHAINED if job["flags"] == "chained" else 0)
    sp = C.c_void_p(stream)
    if job["compress"]:
        rc = lib.lz4flex_compress_batch(ctx, p("src"), p("in_off"), p("in_len"), None, n, p("sink"), p("out_off"), p("cap"), p("out_len"), p("status"), mem, sp)
    else:
        ext = L.DecompressExt(None, None, None, p("pos") if job["pos"] else None, None, 0)
        rc = lib.lz4flex_decompress_batch_ex(ctx, p("src"), p("in_off"), p("in_len"), n, p("sink"), p("out_off"), p("cap"), p("out_len"), p("status"), None,
                                             C.byref(ext), mem, sp)
    return rc


@pytest.mark.parametrize("make,tuning", [(_encode_job, {}), (_chain_job, {}), (_pair_job, {"decompress_pcd_pair": 2})],
                         ids=["throughput-encoder", "chained-decode", "paired-workgroup-decoder"])
def test_two_streams_share_a_workspace(env, make, tuning):
    """two batches back to back on two streams of one context -- both in flight, nothing between the two calls -- give what they give on
    one stream"""
    lib, L, torch = env
    jobs = [make(0), make(1)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    s1, s2 = (s.cuda_stream for s in streams)
    ctx = _ctx(lib, **tuning)
    try:
        staged = [_stage(env, j) for j in jobs + jobs]
        assert [_issue(env, ctx, j, a, s1) for j, a in zip(jobs, staged[:2])] == [0, 0], L.last_error()
        one = [a.fetch() for a in staged[:2]]
        rcs = (_issue(env, ctx, jobs[0], staged[2], s1), _issue(env, ctx, jobs[1], staged[3], s2))
        assert rcs == (0, 0), (rcs, L.last_error())
        two = [a.fetch() for a in staged[2:]]
        for j, a, b in zip(jobs, one, two):
            assert not a["status"].any() and not b["status"].any(), (a["status"], b["status"])
            assert np.array_equal(a["out_len"], b["out_len"])
            if j["compress"]:
                for i in range(8):
                    o, n = int(j["out_off"][i]), int(a["out_len"][i])
                    assert np.array_equal(a["sink"][o:o + n], b["sink"][o:o + n]), i
                    assert O.decompress(b["sink"][o:o + n].tobytes(), 4096) == ("ok", j["src"][4096 * i:4096 * (i + 1)])
            else:
                assert np.array_equal(a["sink"][:j["out_bytes"]], b["sink"][:j["out_bytes"]])
                assert b["sink"][:j["out_bytes"]].tobytes() == j["plain"]
    finally:
        lib.lz4flex_ctx_destroy(ctx)
