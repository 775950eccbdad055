"""GPU: dictionary sets -- K dictionaries prepared once (lz4flex_dict_set_create), one id per block, both directions.

The contract is equality with entries that exist: lz4flex_compress_batch_dict_set gives block i the bytes lz4flex_compress_batch_ex gives
it with dictionary dict_id[i] as its per-block dictionary (fast mode: the scalar model's, tests/dict_cases.py; exact mode: the oracle's
compress_into_with_dict), lz4flex_decompress_batch_dict_set what lz4flex_decompress_batch_ex gives it.  Equal bytes cannot show that a
digest was used, so fast-mode calls also read the set's counter of items whose first window started from a digest and compare it with
the number the header's eligibility rule gives."""
import ctypes as C

import numpy as np
import pytest

import dict_cases as D
import oracle_api as O
import wave_model as W

pytestmark = pytest.mark.gpu

CANARY = 0xA5
PAD = 64
NONE = 0xFFFFFFFF
REDO = 0x7F000001
INVALID = 64
# no dictionary by length; exact mode's tiny dictionary; the last length without a digest and the first with one; a full digest; more
# than the 64 KiB the set keeps
DICT_LENS = [0, 3, 1026, 1027, 31744 + 3, 70000]
DICT_KINDS = ["json", "text", "log", "json", "text", "log"]
BLOCK_LENS = D.LENS + [2, 7, 8, 11, 4095, 4097, 32769]
IDS = [0, 1, 2, 3, 4, 5, NONE]


def eligible(dict_len, block_len, cap):
    """the header's rule: the item [h | block] starts from its dictionary's digest when there is one (hs > 0), the block is encoded at
    all (out_cap at least the maximum output size) and every position below hs may start a match (block length >= hs + 11 - h)"""
    h = min(dict_len, W.HIST)
    hs = (h - 3) // 1024 * 1024 if h >= 1027 else 0
    return hs > 0 and cap >= O.max_out(block_len) and block_len >= hs + 11 - h


def dicts():
    return [D.dictionary(k)[D.DICT_BYTES - n:] if n else b"" for k, n in zip(DICT_KINDS, DICT_LENS)]


def dict_of(ds, i):
    return b"" if i == NONE else ds[i]


def the_batch():
    """every (dictionary, length) pair once, the ids cycling; the short lengths a second time with other data: 182 blocks"""
    ids, blocks = [], []
    for rnd, lens in enumerate((BLOCK_LENS, [n for n in BLOCK_LENS if n < 5000])):
        for j, n in enumerate(lens):
            for i in IDS:
                ids.append(i)
                blocks.append(D.block("json" if i == NONE else DICT_KINDS[i], n, salt=(j + 3 * rnd) % 7))
    return blocks, ids


@pytest.fixture(scope="module")
def env():
    import torch
    from lz4_flex_amd import _lib
    lib = _lib.load()
    assert lib.lz4flex_device_count() >= 1, _lib.last_error()
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
    yield lib, _lib, torch, ctx
    lib.lz4flex_ctx_destroy(ctx)


class tuned:
    """settings of the module's context for the length of a with block"""

    def __init__(self, env, **kv):
        self.env, self.kv = env, kv

    def __enter__(self):
        lib, ctx = self.env[0], self.env[3]
        self.old = {k: lib.lz4flex_get_tuning(ctx, k.encode()) for k in self.kv}
        for k, v in self.kv.items():
            assert lib.lz4flex_set_tuning(ctx, k.encode(), v) == 0, k

    def __exit__(self, *exc):
        lib, ctx = self.env[0], self.env[3]
        for k, v in self.old.items():
            assert lib.lz4flex_set_tuning(ctx, k.encode(), v) == 0, k


def counter(env):
    v = env[0].lz4flex_get_tuning(env[3], b"debug_dict_set_items")
    assert v >= 0, v
    return v


def make_set(env, ds, mem="host", ctx=None):
    """a set of the dictionaries ds, each at an odd offset between canaries in the caller's buffer; the buffer is overwritten with the
    canary once the set exists (the set owns its copy)"""
    lib, L, torch = env[:3]
    off, pos = [], 3
    for d in ds:
        off.append(pos)
        pos += len(d) + 5
    buf = np.full(pos + PAD, CANARY, np.uint8)
    for o, d in zip(off, ds):
        buf[o:o + len(d)] = np.frombuffer(d, np.uint8)
    offs, lens = np.array(off, np.uint64), np.array([len(d) for d in ds], np.uint32)
    h = C.c_void_p()
    if mem == "host":
        rc = lib.lz4flex_dict_set_create(ctx or env[3], C.c_void_p(buf.ctypes.data), C.c_void_p(offs.ctypes.data), C.c_void_p(lens.ctypes.data),
                                         len(ds), L.MEM_HOST, C.byref(h))
        buf[:] = CANARY
    else:
        t = [torch.from_numpy(a.view(np.uint8)).to("cuda") for a in (buf, offs, lens)]
        rc = lib.lz4flex_dict_set_create(ctx or env[3], C.c_void_p(t[0].data_ptr()), C.c_void_p(t[1].data_ptr()), C.c_void_p(t[2].data_ptr()),
                                         len(ds), L.MEM_DEVICE, C.byref(h))
        for a in t:
            a.fill_(CANARY)
        torch.cuda.synchronize()
    assert rc == 0 and h.value, (rc, L.last_error())
    assert lib.lz4flex_dict_set_count(h) == len(ds)
    return h


@pytest.fixture(scope="module")
def the_set(env):
    h = make_set(env, dicts())
    yield h
    env[2].cuda.synchronize()
    env[0].lz4flex_dict_set_free(h)


class Batch:
    """n blocks (to compress, or compressed ones) at odd offsets, output slots of caps[i] bytes between canaries, an id per block"""

    def __init__(self, blocks, ids, caps):
        self.blocks, self.ids_list, self.n = blocks, list(ids), len(blocks)
        in_off, pos = [], 1
        for b in blocks:
            in_off.append(pos)
            pos += len(b) + 3
        self.in_buf = np.full(pos + PAD, CANARY, np.uint8)
        for o, b in zip(in_off, blocks):
            self.in_buf[o:o + len(b)] = np.frombuffer(b, np.uint8)
        out_off, pos = [], 5
        for c in caps:
            out_off.append(pos)
            pos += c + PAD + (1 if (pos + c + PAD) % 16 == 0 else 0)
        self.out_init = np.full(pos, CANARY, np.uint8)
        self.in_off, self.in_len = np.array(in_off, np.uint64), np.array([len(b) for b in blocks], np.uint32)
        self.out_off, self.out_cap = np.array(out_off, np.uint64), np.array(caps, np.uint32)
        self.ids = np.array(ids, np.uint32)

    def ex_arrays(self, ds):
        """the per-block dictionary arrays of the *_ex entries for the same batch (a refused id: no dictionary -- not compared)"""
        off, pos = [], 7
        for d in ds:
            off.append(pos)
            pos += len(d) + 1
        buf = np.full(pos + PAD, CANARY, np.uint8)
        for o, d in zip(off, ds):
            buf[o:o + len(d)] = np.frombuffer(d, np.uint8)
        ok = [i if i != NONE and i < len(ds) else None for i in self.ids_list]
        return (buf, np.array([off[i] if i is not None else 0 for i in ok], np.uint64),
                np.array([len(ds[i]) if i is not None else 0 for i in ok], np.uint32))

    def run(self, env, compress, mem, set_=None, ex=None, ctx=None):
        """one call: the set entry (set_) or the *_ex entry with the per-block arrays `ex`.  Returns (out image, out_len, status, detail);
        the inputs and every byte outside the sinks must be what they were"""
        lib, L, torch = env[:3]
        ctx = ctx or env[3]
        n = self.n
        host = dict(in_buf=self.in_buf.copy(), in_off=self.in_off, in_len=self.in_len, ids=self.ids, out=self.out_init.copy(),
                    out_off=self.out_off, out_cap=self.out_cap, out_len=np.full(n, 0xDEAD, np.uint32), status=np.full(n, -1, np.int32),
                    detail=np.full(2 * n, 0xEE, np.uint64))
        if ex is not None:
            host.update(dbuf=ex[0].copy(), doff=ex[1], dlen=ex[2])
        if mem == "host":
            keep, kind, sp = host, L.MEM_HOST, None
            p = {k: C.c_void_p(v.ctypes.data) for k, v in host.items()}
        else:
            keep = {k: torch.from_numpy(v.view(np.uint8)).to("cuda") for k, v in host.items()}
            p = {k: C.c_void_p(v.data_ptr()) for k, v in keep.items()}
            big = int(self.in_len.max(initial=0)) > (65536 if compress else 131072)
            kind, sp = L.MEM_DEVICE | (L.MEM_BIG_BLOCKS if big else 0), C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if set_ is not None and compress:
            rc = lib.lz4flex_compress_batch_dict_set(ctx, p["in_buf"], p["in_off"], p["in_len"], n, p["ids"], p["out"], p["out_off"], p["out_cap"],
                                                     p["out_len"], p["status"], set_, kind, sp)
        elif set_ is not None:
            rc = lib.lz4flex_decompress_batch_dict_set(ctx, p["in_buf"], p["in_off"], p["in_len"], n, p["ids"], p["out"], p["out_off"], p["out_cap"],
                                                       p["out_len"], p["status"], p["detail"], set_, kind, sp)
        elif compress:
            e = L.CompressExt(p["dbuf"], p["doff"], p["dlen"])
            rc = lib.lz4flex_compress_batch_ex(ctx, p["in_buf"], p["in_off"], p["in_len"], None, n, p["out"], p["out_off"], p["out_cap"],
                                               p["out_len"], p["status"], C.byref(e), kind, sp)
        else:
            e = L.DecompressExt(p["dbuf"], p["doff"], p["dlen"], None, None, 0)
            rc = lib.lz4flex_decompress_batch_ex(ctx, p["in_buf"], p["in_off"], p["in_len"], n, p["out"], p["out_off"], p["out_cap"],
                                                 p["out_len"], p["status"], p["detail"], C.byref(e), kind, sp)
        assert rc == 0, (rc, L.last_error())
        if mem != "host":
            torch.cuda.synchronize()
            for k in ("in_buf", "out", "out_len", "status", "detail") + (("dbuf",) if ex is not None else ()):
                host[k].view(np.uint8)[:] = keep[k].cpu().numpy()
        assert np.array_equal(host["in_buf"], self.in_buf), "the input (or a canary around it) was written"
        if ex is not None:
            assert np.array_equal(host["dbuf"], ex[0]), "a dictionary (or a canary around one) was written"
        out, out_len, status = host["out"], host["out_len"], host["status"]
        inside = np.zeros(len(out), bool)
        for i in range(n):
            o, c, m = int(self.out_off[i]), int(self.out_cap[i]), int(out_len[i])
            if status[i] == 0:
                assert m <= c, i
                inside[o:o + (m if compress else c)] = True        # (a decoder may rewrite the rest of its sink, never a byte behind it)
            else:
                assert m == 0, (i, status[i])
                if mem != "host" and status[i] != INVALID:
                    inside[o:o + c] = True                            # a failed block may have written part of its sink (device memory)
        assert (out[~inside] == CANARY).all(), "bytes outside the sinks (or in the slot of a refused / failed block) were written"
        return out, out_len, status, host["detail"].reshape(n, 2)

    def outputs(self, res):
        return [bytes(res[0][int(o):int(o) + int(m)]) for o, m in zip(self.out_off, res[1])]


_made = {}


def compress_batch():
    if "c" not in _made:
        blocks, ids = the_batch()
        _made["c"] = Batch(blocks, ids, [O.max_out(len(b)) for b in blocks])
    return _made["c"]


def n_eligible(batch, ds):
    return sum(eligible(len(dict_of(ds, i)), len(b), int(c)) for b, i, c in zip(batch.blocks, batch.ids_list, batch.out_cap))


def models(batch, ds):
    if "m" not in _made:
        _made["m"] = [D.model(b, dict_of(ds, i)) if len(dict_of(ds, i)) else None for b, i in zip(batch.blocks, batch.ids_list)]
    return _made["m"]


# ---------------------------------------------------------------- compress
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("sliding", [0, 1, 2])
def test_fast_equals_batch_ex_and_the_model(env, the_set, sliding, mem):
    ds, b = dicts(), compress_batch()
    with tuned(env, compress_mode=0, compress_sliding_window=sliding):
        got = b.run(env, True, mem, set_=the_set)
        items = counter(env)
        ref = b.run(env, True, mem, ex=b.ex_arrays(ds))
    assert (got[2] == 0).all() and (ref[2] == 0).all(), (got[2], ref[2])
    assert items == n_eligible(b, ds) and items > 0
    outs, want = b.outputs(got), b.outputs(ref)
    bad = [(i, b.ids_list[i], len(b.blocks[i])) for i in range(b.n) if outs[i] != want[i]]
    assert not bad, bad[:8]
    # (a dictionary item's windows advance by HIST under every setting: the model's bytes hold for all three)
    bad = [(i, b.ids_list[i], len(b.blocks[i])) for i, m in enumerate(models(b, ds)) if m is not None and outs[i] != m]
    assert not bad, bad[:8]
    _made[("fast", sliding)] = outs


@pytest.mark.parametrize("mem", ["host", "device"])
def test_fast_without_digests_same_bytes(env, the_set, mem):
    ds, b = dicts(), compress_batch()
    with tuned(env, compress_mode=0, compress_shared_dict=0):
        got = b.run(env, True, mem, set_=the_set)
        assert counter(env) == 0
        ref = b.run(env, True, mem, ex=b.ex_arrays(ds))
    assert (got[2] == 0).all()
    assert b.outputs(got) == b.outputs(ref)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_exact_equals_batch_ex_and_the_oracle(env, the_set, mem):
    ds, b = dicts(), compress_batch()
    with tuned(env, compress_mode=1):
        got = b.run(env, True, mem, set_=the_set)
        assert counter(env) == 0
        ref = b.run(env, True, mem, ex=b.ex_arrays(ds))
    assert (got[2] == 0).all() and (ref[2] == 0).all()
    outs = b.outputs(got)
    assert outs == b.outputs(ref)
    for i in range(b.n):
        d = dict_of(ds, b.ids_list[i])
        assert outs[i] == (O.compress_with_dict(b.blocks[i], d) if len(d) else O.compress(b.blocks[i])), (i, b.ids_list[i], len(b.blocks[i]))
    _made["exact"] = outs


def test_a_set_outlives_a_shared_dictionary_call(env, the_set):
    """the set's digests are not in the workspace a lz4flex_compress_batch_shared_dict call on the same context writes its digest to"""
    lib, L = env[0], env[1]
    b = compress_batch()
    with tuned(env, compress_mode=0):
        first = b.outputs(b.run(env, True, "device", set_=the_set))
        other = np.frombuffer(D.dictionary("random")[:40000], np.uint8).copy()
        one = Batch([D.block("text", 4096)], [0], [O.max_out(4096)])
        ol, st = np.zeros(1, np.uint32), np.zeros(1, np.int32)
        p = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731
        out = one.out_init.copy()
        assert lib.lz4flex_compress_batch_shared_dict(env[3], p(one.in_buf), p(one.in_off), p(one.in_len), 1, p(out), p(one.out_off), p(one.out_cap),
                                                      p(ol), p(st), p(other), len(other), L.MEM_HOST, None) == 0 and st[0] == 0
        second = b.run(env, True, "device", set_=the_set)
        assert counter(env) == n_eligible(b, dicts())
    assert b.outputs(second) == first


@pytest.mark.parametrize("mem", ["host", "device"])
def test_the_set_owns_its_bytes(env, the_set, mem):
    """make_set overwrites the caller's buffers once the set exists: a HOST-created and a DEVICE-created set give what the module's gives"""
    blocks, ids = the_batch()
    keep = [i for i in range(len(blocks)) if len(blocks[i]) <= 4097]
    b = Batch([blocks[i] for i in keep], [ids[i] for i in keep], [O.max_out(len(blocks[i])) for i in keep])
    h = make_set(env, dicts(), mem)
    try:
        with tuned(env, compress_mode=0):
            a = b.run(env, True, "device", set_=h)
            c = b.run(env, True, "device", set_=the_set)
        assert (a[2] == 0).all() and b.outputs(a) == b.outputs(c)
        comp = b.outputs(a)
        d = Batch(comp, b.ids_list, [len(x) for x in b.blocks])
        r = d.run(env, False, "device", set_=h)
        assert (r[2] == 0).all() and d.outputs(r) == b.blocks
    finally:
        env[2].cuda.synchronize()
        env[0].lz4flex_dict_set_free(h)


# ---------------------------------------------------------------- decompress
def valid_batch(env, the_set):
    """what the compress tests produced (this library's bytes in both modes, which are the oracle's in exact mode), every block against
    its own dictionary, sinks of exactly the block's size"""
    if "v" not in _made:
        b = compress_batch()
        for key, mode in ((("fast", 2), 0), ("exact", 1)):
            if key not in _made:
                with tuned(env, compress_mode=mode):
                    _made[key] = b.outputs(b.run(env, True, "device", set_=the_set))
        comp = _made[("fast", 2)] + _made["exact"]
        _made["v"] = Batch(comp, b.ids_list * 2, [len(x) for x in b.blocks] * 2)
        _made["v_plain"] = b.blocks * 2
    return _made["v"], _made["v_plain"]


def same(a, b, n, what):
    assert np.array_equal(a[1], b[1]), (what, "out_len", np.nonzero(a[1] != b[1])[0][:8])
    assert np.array_equal(a[2], b[2]), (what, "status", np.nonzero(a[2] != b[2])[0][:8], a[2][a[2] != b[2]][:8], b[2][a[2] != b[2]][:8])
    assert np.array_equal(a[3], b[3]), (what, "detail")


@pytest.mark.parametrize("mem", ["host", "device"])
def test_valid_blocks_equal_batch_ex(env, the_set, mem):
    v, plain = valid_batch(env, the_set)
    got = v.run(env, False, mem, set_=the_set)
    ref = v.run(env, False, mem, ex=v.ex_arrays(dicts()))
    assert (got[2] == 0).all(), np.nonzero(got[2])[0][:8]
    same(got, ref, v.n, mem)
    assert v.outputs(got) == plain
    assert (got[3] == 0).all()


def lits(n, seed):
    return bytes((seed * 31 + 7 * i) % 251 for i in range(n))


def seq(lit, off, ml):
    """a sequence: token, literals, offset, match length (ml 4 ... 18)"""
    assert len(lit) < 15 and 4 <= ml < 19
    return bytes([(len(lit) << 4) | (ml - 4)]) + lit + bytes([off & 255, off >> 8])


def last(lit):
    return bytes([len(lit) << 4]) + lit


def hostile(ds):
    """per dictionary: (name, block, cap, id)"""
    cases = []
    for i in IDS:
        dl = len(dict_of(ds, i))
        reach = min(4 + dl, 65535)
        ok = seq(lits(4, i), reach, 8) + last(lits(5, 9))                       # 17 bytes; the match begins at the dictionary's first kept byte
        cases += [("reach", ok, 17, i),
                  ("reach + 1", seq(lits(4, i), min(reach + 1, 65535), 8) + last(lits(5, 9)), 17, i),     # OffsetOutOfBounds where an offset can say it
                  ("offset 0", seq(lits(4, i), 0, 8) + last(lits(5, 9)), 17, i),
                  ("literals cut", ok[:3], 17, i),
                  ("offset cut", ok[:6], 17, i),
                  ("length byte missing", bytes([0x4F]) + lits(4, i) + bytes([4 if dl else 1, 0]), 64, i),
                  ("empty", b"", 17, i),
                  ("cap one short", ok, 16, i),
                  ("cap cuts the match", ok, 11, i),
                  ("cap 0", ok, 0, i),
                  ("across", seq(lits(4, i), 6, 12) + last(lits(5, 3)), 21, i),       # 2 bytes of the dictionary, then the block's own
                  ("across, long", seq(lits(4, i), 6, 18) + seq(lits(3, 5), 7, 18) + last(lits(5, 3)), 48, i)]
        if dl >= 65535:
            cases.append(("distance 65 535", seq(b"", 65535, 18) + seq(lits(1, 2), 65535, 18) + last(lits(5, 1)), 42, i))
    return cases


def hostile_batch():
    if "h" not in _made:
        cases = hostile(dicts())
        _made["h"] = (Batch([c[1] for c in cases], [c[3] for c in cases], [c[2] for c in cases]), cases)
    return _made["h"]


def test_hostile_cases_say_what_they_mean():
    ds = dicts()
    want = {"offset 0": "OffsetZero", "literals cut": "LiteralOutOfBounds", "offset cut": "ExpectedAnotherByte", "empty": "ExpectedAnotherByte",
            "cap one short": "OutputTooSmall", "cap cuts the match": "OutputTooSmall", "cap 0": "OutputTooSmall",
            "length byte missing": "ExpectedAnotherByte", "reach": "ok", "distance 65 535": "ok"}
    for name, blk, cap, i in hostile(ds):
        d = dict_of(ds, i)
        verdict = O.decompress(blk, cap, dict_data=d)[0]
        if name in want:
            assert verdict == want[name], (name, i, verdict)
        if name == "reach + 1":
            assert verdict == ("OffsetOutOfBounds" if len(d) < 65531 else "ok"), (i, verdict)
        if name.startswith("across"):
            assert verdict == ("ok" if len(d) >= 2 else "OffsetOutOfBounds"), (name, i, verdict)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_hostile_blocks_equal_batch_ex(env, the_set, mem):
    ds = dicts()
    h, cases = hostile_batch()
    got = h.run(env, False, mem, set_=the_set)
    ref = h.run(env, False, mem, ex=h.ex_arrays(ds))
    same(got, ref, h.n, mem)
    for k, (name, blk, cap, i) in enumerate(cases):
        w = O.decompress(blk, cap, dict_data=dict_of(ds, i))
        if w[0] == "ok":
            assert got[2][k] == 0 and h.outputs(got)[k] == w[1], (name, i)
        else:
            assert O.ERR_NAMES[int(got[2][k])] == w[0], (name, i, got[2][k], w)
            assert tuple(int(x) for x in got[3][k]) == ((w[1][0], cap) if w[0] == "OutputTooSmall" else (0, 0)), (name, i)


def test_kernel_and_fallback(env, the_set):
    """second pass off: the sequence decoder itself decoded the valid blocks (status 0, not the marker) and handed the failing ones back;
    "decompress_variant" 1 (every block in the reference's order): the same results"""
    v, plain = valid_batch(env, the_set)
    h, cases = hostile_batch()
    ds = dicts()
    full_v, full_h = v.run(env, False, "device", set_=the_set), h.run(env, False, "device", set_=the_set)
    with tuned(env, decompress_second_pass=0):
        r = v.run(env, False, "device", set_=the_set)
        assert (r[2] == 0).all(), np.nonzero(r[2])[0][:8]
        assert v.outputs(r) == plain
        r = h.run(env, False, "device", set_=the_set)
        for k, (name, blk, cap, i) in enumerate(cases):
            ok = O.decompress(blk, cap, dict_data=dict_of(ds, i))[0] == "ok"
            assert int(r[2][k]) in ((0, REDO) if ok else (REDO,)), (name, i, hex(int(r[2][k])))
    for setting in (dict(decompress_variant=1), dict(decompress_shared_dict=0)):
        with tuned(env, **setting):
            r = v.run(env, False, "device", set_=the_set)
            same(r, full_v, v.n, setting)
            assert v.outputs(r) == plain
            same(h.run(env, False, "device", set_=the_set), full_h, h.n, setting)


# ---------------------------------------------------------------- ids the set does not have
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("mode", [0, 1])
def test_refused_ids(env, the_set, mode, mem):
    ds = dicts()
    blocks = [D.block("json", n, salt=j) for j, n in enumerate([4096, 100, 4096, 0, 4097, 4096, 12])]
    ids = [4, len(ds), 5, 0xFFFFFFFE, NONE, len(ds) + 1000, 3]
    good = [k for k, i in enumerate(ids) if i == NONE or i < len(ds)]
    b = Batch(blocks, ids, [O.max_out(len(x)) for x in blocks])
    with tuned(env, compress_mode=mode):
        got = b.run(env, True, mem, set_=the_set)           # (run: nothing in the slot of a block with status INVALID_ARG is written)
        ref = b.run(env, True, mem, ex=b.ex_arrays(ds))
    assert [int(s) for s in got[2]] == [0 if k in good else INVALID for k in range(b.n)]
    outs = b.outputs(got)
    assert [outs[k] for k in good] == [b.outputs(ref)[k] for k in good]
    comp = [outs[k] if k in good else O.compress(blocks[k]) for k in range(b.n)]
    d = Batch(comp, ids, [len(x) for x in blocks])
    for setting in (dict(), dict(decompress_variant=1)):
        with tuned(env, **setting):
            r = d.run(env, False, mem, set_=the_set)
        assert [int(s) for s in r[2]] == [0 if k in good else INVALID for k in range(b.n)], setting
        assert (r[3][[k for k in range(b.n) if k not in good]] == 0).all()
        assert [d.outputs(r)[k] for k in good] == [blocks[k] for k in good]


# ---------------------------------------------------------------- K = 1: the *_shared_dict entries
@pytest.mark.parametrize("kind,dlen", [("json", 40000), ("zero", 40000), ("text", 1027)])
def test_a_set_of_one_equals_the_shared_entries(env, kind, dlen):
    lib, L, torch, ctx = env
    d = D.dictionary(kind)[D.DICT_BYTES - dlen:]
    blocks = [D.block(k, n, salt=j) for j, (k, n) in enumerate([(kind, 4096), (kind, 8), (kind, 7), ("zero", 32769), (kind, 65537), (kind, 0)])]
    b = Batch(blocks, [0] * len(blocks), [O.max_out(len(x)) for x in blocks])
    h = make_set(env, [d], "device")
    try:
        with tuned(env, compress_mode=0):
            got = b.run(env, True, "device", set_=h)
            items = counter(env)
            t = {k: torch.from_numpy(v.view(np.uint8)).to("cuda") for k, v in
                 dict(i=b.in_buf, io=b.in_off, il=b.in_len, o=b.out_init, oo=b.out_off, oc=b.out_cap, d=np.frombuffer(d, np.uint8).copy()).items()}
            ol, st = torch.zeros(b.n, dtype=torch.int32, device="cuda"), torch.full((b.n,), -1, dtype=torch.int32, device="cuda")
            q = lambda x: C.c_void_p(x.data_ptr())      # noqa: E731
            sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            assert lib.lz4flex_compress_batch_shared_dict(ctx, q(t["i"]), q(t["io"]), q(t["il"]), b.n, q(t["o"]), q(t["oo"]), q(t["oc"]), q(ol), q(st),
                                                          q(t["d"]), len(d), L.MEM_DEVICE | L.MEM_BIG_BLOCKS, sp) == 0
            torch.cuda.synchronize()
            assert items == lib.lz4flex_get_tuning(ctx, b"debug_shared_dict_items")
        assert (got[2] == 0).all() and (st == 0).all()
        assert np.array_equal(got[0], t["o"].cpu().numpy()), "the output images differ"
        assert np.array_equal(got[1], ol.cpu().numpy().view(np.uint32))
        comp = b.outputs(got)
        dd = Batch(comp + [comp[0][:-3]], [0] * (b.n + 1), [len(x) for x in blocks] + [4096])
        r = dd.run(env, False, "device", set_=h)
        t = {k: torch.from_numpy(v.view(np.uint8)).to("cuda") for k, v in
             dict(i=dd.in_buf, io=dd.in_off, il=dd.in_len, o=dd.out_init, oo=dd.out_off, oc=dd.out_cap, d=np.frombuffer(d, np.uint8).copy()).items()}
        ol, st = torch.zeros(dd.n, dtype=torch.int32, device="cuda"), torch.full((dd.n,), -1, dtype=torch.int32, device="cuda")
        det = torch.zeros(2 * dd.n, dtype=torch.int64, device="cuda")
        assert lib.lz4flex_decompress_batch_shared_dict(ctx, q(t["i"]), q(t["io"]), q(t["il"]), dd.n, q(t["o"]), q(t["oo"]), q(t["oc"]), q(ol), q(st),
                                                        q(det), q(t["d"]), len(d), L.MEM_DEVICE, sp) == 0
        torch.cuda.synchronize()
        assert np.array_equal(r[2], st.cpu().numpy()) and np.array_equal(r[1], ol.cpu().numpy().view(np.uint32))
        assert np.array_equal(r[3].reshape(-1), det.cpu().numpy().view(np.uint64))
        assert dd.outputs(r)[:b.n] == blocks and r[2][b.n] != 0
    finally:
        torch.cuda.synchronize()
        lib.lz4flex_dict_set_free(h)


# ---------------------------------------------------------------- Python
def test_python_round_trip(env):
    import torch
    from lz4_flex_amd import block
    ds = dicts()
    blocks, ids = the_batch()
    keep = [i for i in range(len(blocks)) if len(blocks[i]) <= 65537][:60] + [0]
    blocks, ids = [blocks[i] for i in keep], [ids[i] for i in keep]
    ids[-1] = len(ds)                                   # one id the set does not have
    src = torch.from_numpy(np.frombuffer(b"".join(blocks) + b"\0", np.uint8).copy()).to("cuda")
    lens = torch.tensor([len(b) for b in blocks], dtype=torch.int64)
    offs = torch.cumsum(lens, 0) - lens
    tid = torch.tensor(ids, dtype=torch.int64)
    with block.DictSet(ds) as s:
        assert len(s) == len(ds)
        out, out_off, out_len, status = block.compress_blocks_with_dict_set_device(src, offs, lens, tid, s)
        assert status.tolist() == [0] * (len(blocks) - 1) + [INVALID]
        back, b_off, b_len, b_st = block.decompress_blocks_with_dict_set_device(out, out_off, out_len, tid, s)
        torch.cuda.synchronize()
        assert b_st.tolist() == [0] * (len(blocks) - 1) + [INVALID]
        back, b_off, b_len = back.cpu().numpy(), b_off.tolist(), b_len.tolist()
        for k, b in enumerate(blocks[:-1]):
            assert b_len[k] == len(b) and bytes(back[b_off[k]:b_off[k] + b_len[k]]) == b, k
        # the host forms against the per-block entry
        n = len(blocks) - 1
        caps = np.array([O.max_out(len(b)) for b in blocks[:n]], np.uint32)
        coff = (np.cumsum(caps, dtype=np.uint64) - caps).astype(np.uint64)
        ob = np.zeros(int(caps.sum()) + 1, np.uint8)
        hl, hs = block.compress_batch_with_dict_set(src.cpu().numpy(), offs.numpy()[:n], lens.numpy()[:n], ids[:n], s, ob, coff, caps)
        assert (hs == 0).all() and hl.tolist() == out_len.tolist()[:n]
        oc = np.array([len(b) for b in blocks[:n]], np.uint32)
        oo = (np.cumsum(oc, dtype=np.uint64) - oc).astype(np.uint64)
        plain = np.zeros(int(oc.sum()) + 1, np.uint8)
        dl, dst, _ = block.decompress_batch_with_dict_set(ob, coff, hl, ids[:n], s, plain, oo, oc)
        assert (dst == 0).all() and bytes(plain[:-1]) == b"".join(blocks[:n])
    with pytest.raises(ValueError):
        s.handle
    s.close()
