"""GPU: lz4flex_compress_batch_ex -- blocks compressed against per-block dictionaries, in both compress modes.

fast (the throughput encoder): every block's bytes equal the scalar model's for the item [dictionary tail | block]
(tests/dict_cases.py), whatever the batch shape, the memory kind or the carry wait; exact: the oracle's compress_into_with_dict.
Every block is decoded by the oracle and by lz4flex_decompress_batch_ex with its dictionary; canaries sit behind every out_cap."""
import ctypes as C

import numpy as np
import pytest

import dict_cases as D
import oracle_api as O

pytestmark = pytest.mark.gpu

CANARY = 0xA5
PAD = 64


def _lib():
    from lz4_flex_amd import _lib
    return _lib


def _mode(m):
    from lz4_flex_amd import block
    block.set_compress_mode(m)


@pytest.fixture
def fast():
    _mode("fast")
    yield
    _mode("fast")


@pytest.fixture
def exact():
    _mode("exact")
    yield
    _mode("fast")


def _tuning(key, v):
    L = _lib()
    assert L.load().lz4flex_set_tuning(None, key.encode(), v) == 0


def layout(blocks, dict_buf, dict_off, dict_len, caps=None, odd=True):
    """in_buf / out_buf with odd offsets and a canary region of PAD bytes behind every out_cap"""
    in_off, pos = [], 1 if odd else 0
    for b in blocks:
        in_off.append(pos)
        pos += len(b) + (3 if odd else 0)
    in_buf = np.zeros(pos + 16, np.uint8)
    for o, b in zip(in_off, blocks):
        in_buf[o:o + len(b)] = np.frombuffer(b, np.uint8)
    caps = [O.max_out(len(b)) for b in blocks] if caps is None else caps
    out_off, pos = [], 5 if odd else 0
    for c in caps:
        out_off.append(pos)
        pos += c + PAD
    out_buf = np.full(pos, CANARY, np.uint8)
    return dict(in_buf=in_buf, in_off=np.array(in_off, np.uint64), in_len=np.array([len(b) for b in blocks], np.uint32),
                dict_buf=np.ascontiguousarray(dict_buf, np.uint8), dict_off=np.array(dict_off, np.uint64),
                dict_len=np.array(dict_len, np.uint32), out_buf=out_buf, out_off=np.array(out_off, np.uint64),
                out_cap=np.array(caps, np.uint32))


def run(lay, mem="host", flags=None, ext=True, dict_base_null=False, dict_is_input=False):
    """one lz4flex_compress_batch_ex; returns (outputs[list of bytes], out_len, status); checks every canary"""
    import torch
    L = _lib()
    lib = L.load()
    n = len(lay["in_off"])
    fl = None if flags is None else np.array(flags, np.uint32)
    if mem == "host":
        arrs = lay
        p = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731
        out_len = np.zeros(n, np.uint32)
        status = np.full(n, -1, np.int32)
        dbase = lay["in_buf"].ctypes.data if dict_is_input else lay["dict_buf"].ctypes.data
        e = L.CompressExt(None if dict_base_null else dbase, arrs["dict_off"].ctypes.data, arrs["dict_len"].ctypes.data)
        rc = lib.lz4flex_compress_batch_ex(None, p(arrs["in_buf"]), p(arrs["in_off"]), p(arrs["in_len"]), p(fl) if fl is not None else None,
                                           n, p(arrs["out_buf"]), p(arrs["out_off"]), p(arrs["out_cap"]), p(out_len), p(status),
                                           C.byref(e) if ext else None, L.MEM_HOST, None)
        assert rc == 0, (rc, L.last_error())
        out_buf = lay["out_buf"]
    else:
        dev = torch.device("cuda")
        t = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else (v.view(np.int32) if v.dtype == np.uint32 else v)).to(dev)
             for k, v in lay.items()}
        tf = torch.from_numpy(fl.view(np.int32)).to(dev) if fl is not None else None
        out_len = torch.zeros(n, dtype=torch.int32, device=dev)
        status = torch.full((n,), -1, dtype=torch.int32, device=dev)
        q = lambda x: C.c_void_p(x.data_ptr())        # noqa: E731
        dbase = t["in_buf"].data_ptr() if dict_is_input else t["dict_buf"].data_ptr()
        e = L.CompressExt(None if dict_base_null else dbase, t["dict_off"].data_ptr(), t["dict_len"].data_ptr())
        big = L.MEM_BIG_BLOCKS if int(lay["in_len"].max(initial=0)) > 65536 else 0
        s = torch.cuda.current_stream().cuda_stream
        rc = lib.lz4flex_compress_batch_ex(None, q(t["in_buf"]), q(t["in_off"]), q(t["in_len"]), q(tf) if tf is not None else None, n,
                                           q(t["out_buf"]), q(t["out_off"]), q(t["out_cap"]), q(out_len), q(status),
                                           C.byref(e) if ext else None, L.MEM_DEVICE | big, C.c_void_p(s))
        assert rc == 0, (rc, L.last_error())
        torch.cuda.synchronize()
        out_buf = t["out_buf"].cpu().numpy()
        lay["out_buf"][:] = out_buf
        out_len = out_len.cpu().numpy().view(np.uint32)
        status = status.cpu().numpy()
    outs = []
    for i in range(n):
        o, c, m = int(lay["out_off"][i]), int(lay["out_cap"][i]), int(out_len[i])
        if status[i] != 0:
            assert m == 0
            assert (out_buf[o:o + c + PAD] == CANARY).all(), "block %d (status %d) wrote bytes" % (i, status[i])
        else:
            assert (out_buf[o + m:o + c + PAD] == CANARY).all(), "block %d wrote behind its length" % i
        outs.append(bytes(out_buf[o:o + m]))
    return outs, out_len, status


def decode_check(lay, outs, status, dict_src=None):
    """every good block: the oracle with its dictionary, and lz4flex_decompress_batch_ex with its dictionary, return it"""
    from lz4_flex_amd import block
    dsrc = lay["dict_buf"] if dict_src is None else dict_src
    good = [i for i in range(len(outs)) if status[i] == 0]
    blocks = [bytes(lay["in_buf"][int(lay["in_off"][i]):int(lay["in_off"][i]) + int(lay["in_len"][i])]) for i in good]
    dicts = [bytes(dsrc[int(lay["dict_off"][i]):int(lay["dict_off"][i]) + int(lay["dict_len"][i])]) for i in good]
    for i, b, d in zip(good, blocks, dicts):
        st, got = O.decompress(outs[i], len(b), dict_data=d if d else None)
        assert st == "ok" and got == b, i
    if not good:
        return
    comp = np.frombuffer(b"".join(outs[i] for i in good) + b"\0", np.uint8)
    coff = np.cumsum([0] + [len(outs[i]) for i in good[:-1]]).astype(np.uint64)
    clen = np.array([len(outs[i]) for i in good], np.uint32)
    ooff = np.cumsum([0] + [len(b) for b in blocks[:-1]]).astype(np.uint64)
    ocap = np.array([len(b) for b in blocks], np.uint32)
    out = np.zeros(int(ocap.sum()) + 1, np.uint8)
    ol, st, _ = block.decompress_batch_with_dict(comp, coff, clen, dsrc, lay["dict_off"][good], lay["dict_len"][good], out, ooff, ocap)
    assert (st == 0).all(), st
    for k, b in enumerate(blocks):
        assert int(ol[k]) == len(b) and bytes(out[int(ooff[k]):int(ooff[k]) + len(b)]) == b, good[k]


def cases(kind, lens=D.LENS, hs=D.HS):
    """every (h, length) of a kind against one buffer that holds the 1 MiB dictionary at an odd offset: block (h, n)'s dictionary is
    its last h bytes (the whole dictionary for h == HIST) -- dictionaries that overlap each other"""
    d = D.dictionary(kind)
    dict_buf = np.zeros(len(d) + 8, np.uint8)
    dict_buf[3:3 + len(d)] = np.frombuffer(d, np.uint8)
    blocks, doff, dlen, want = [], [], [], []
    for n in lens:
        for j, h in enumerate(hs):
            b = D.block(kind, n, salt=j)
            full = h == hs[-1]
            blocks.append(b)
            doff.append(3 if full else 3 + len(d) - h)
            dlen.append(len(d) if full else h)
            want.append(D.model(b, d if full else d[-h:]))
    return blocks, dict_buf, doff, dlen, want


@pytest.mark.parametrize("kind", D.KINDS)
def test_fast_equals_model_host(fast, kind):
    blocks, dict_buf, doff, dlen, want = cases(kind)
    lay = layout(blocks, dict_buf, doff, dlen)
    outs, _, st = run(lay, "host")
    assert (st == 0).all(), st
    bad = [(i, len(outs[i]), len(want[i])) for i in range(len(want)) if outs[i] != want[i]]
    assert not bad, bad[:8]
    decode_check(lay, outs, st)


@pytest.mark.parametrize("carry_wait", [1, 0])
@pytest.mark.parametrize("kind", ["json", "log", "random"])
def test_fast_equals_model_device(fast, kind, carry_wait):
    """MEM_DEVICE; few large blocks (window mode: the windows of one item are drawn by different workgroups) and all shapes"""
    _tuning("compress_carry_wait", carry_wait)
    try:
        for lens, hs in ((D.LENS, D.HS), ([1 << 20, 300001], [1, 513, 32767, 32768])):
            blocks, dict_buf, doff, dlen, want = cases(kind, lens, hs)
            lay = layout(blocks, dict_buf, doff, dlen)
            outs, _, st = run(lay, "device")
            assert (st == 0).all(), st
            bad = [i for i in range(len(want)) if outs[i] != want[i]]
            assert not bad, bad[:8]
            decode_check(lay, outs, st)
    finally:
        _tuning("compress_carry_wait", 1)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_fast_big_batch_one_shared_dictionary(fast, mem):
    """2 304 log records against one dictionary (every dict_off the same): block mode, the same bytes as the model"""
    d = D.stream("log", 40000, 5_000_000)
    lens = [4096, 1, 12, 13, 700, 65536, 20000, 0]
    blocks = [D.block("log", lens[i % len(lens)], salt=i) for i in range(2304)]
    lay = layout(blocks, np.frombuffer(d, np.uint8), [0] * len(blocks), [len(d)] * len(blocks))
    outs, _, st = run(lay, mem)
    assert (st == 0).all()
    for i in range(0, len(blocks), 7):
        assert outs[i] == D.model(blocks[i], d), i
    decode_check(lay, outs, st)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_fast_dictionaries_inside_the_inputs(fast, mem):
    """dict_base == in_base: every block's dictionary is the block in front of it (and overlaps other blocks' dictionaries)"""
    base = D.stream("json", 64 * 20011 + 9, 12345)
    blocks = [base[1 + 20011 * i:1 + 20011 * i + 20000] for i in range(64)]
    lay = layout(blocks, np.zeros(1, np.uint8), [0] * 64, [0] * 64, odd=True)
    # the dictionary of block i: the bytes of in_buf in front of it (block i - 1 and its gap), any length up to 30 000
    doff, dlen = [], []
    for i in range(64):
        o = int(lay["in_off"][i])
        k = min(o, [1, 5, 4096, 30000][i % 4])
        doff.append(o - k)
        dlen.append(k)
    lay["dict_off"] = np.array(doff, np.uint64)
    lay["dict_len"] = np.array(dlen, np.uint32)
    outs, _, st = run(lay, mem, dict_is_input=True)
    assert (st == 0).all()
    ib = lay["in_buf"]
    for i in range(64):
        d = bytes(ib[doff[i]:doff[i] + dlen[i]])
        assert outs[i] == D.model(blocks[i], d), i
    decode_check(lay, outs, st, dict_src=ib)


def test_fast_h32768_equals_linked_history(fast):
    """h == 32 768: the bytes of lz4flex_compress_batch with LZ4FLEX_BLOCK_HISTORY(32768) and the dictionary tail in front of the block"""
    from lz4_flex_amd import block
    for kind in ("json", "text", "log"):
        d = D.dictionary(kind)
        blocks = [D.block(kind, n, salt=3) for n in (1, 4096, 65536, 65537, 200000)]
        lay = layout(blocks, np.frombuffer(d, np.uint8), [0] * len(blocks), [len(d)] * len(blocks))
        outs, _, st = run(lay, "host")
        assert (st == 0).all()
        items = [d[-32768:] + b for b in blocks]
        ioff = np.cumsum([0] + [len(x) for x in items[:-1]]).astype(np.uint64)
        buf = np.frombuffer(b"".join(items), np.uint8)
        caps = np.array([O.max_out(len(b)) for b in blocks], np.uint32)
        ooff = np.cumsum([0] + list(caps[:-1])).astype(np.uint64)
        ob = np.zeros(int(caps.sum()), np.uint8)
        ol, st2 = block.compress_batch(buf, ioff + 32768, [len(b) for b in blocks], ob, ooff, caps, flags=[32768 << 8] * len(blocks))
        assert (st2 == 0).all()
        for i in range(len(blocks)):
            assert bytes(ob[int(ooff[i]):int(ooff[i]) + int(ol[i])]) == outs[i], (kind, i)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_exact_equals_oracle(exact, mem):
    """compress_mode exact: the oracle's compress_into_with_dict for dictionaries of 1 B ... 1 MiB, blocks up to 1 MiB, both sides of
    the table-kind boundary dict_len + in_len = 65 534 / 65 535; blocks without a dictionary in the same batch"""
    d = D.dictionary("json")
    pairs = [(1, 4096), (3, 100), (4, 13), (100, 65536), (65536, 4096), (65537, 300000), (1 << 20, 1 << 20), (0, 5000), (30000, 0),
             (1000, 64534), (1000, 64535), (65534, 0), (65535, 0), (5, 65530), (4, 65530), (0, 70000)]
    blocks, doff, dlen = [], [], []
    for j, (k, n) in enumerate(pairs):
        blocks.append(D.block("json", n, salt=j))
        doff.append(len(d) - k if k else 12345)
        dlen.append(k)
    lay = layout(blocks, np.frombuffer(d, np.uint8), doff, dlen)
    outs, _, st = run(lay, mem)
    assert (st == 0).all(), st
    for j, (k, n) in enumerate(pairs):
        want = O.compress_with_dict(blocks[j], d[len(d) - k:]) if k else O.compress(blocks[j])
        assert outs[j] == want, (k, n)
    decode_check(lay, outs, st)


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("mem", ["host", "device"])
def test_without_dictionaries_bytes_unchanged(mode, mem):
    """ext NULL, dict_base NULL, every dict_len 0: lz4flex_compress_batch's bytes; a mixed batch gives its dictionary-less blocks
    their plain bytes (a batch of the same size)"""
    _mode(mode)
    try:
        blocks = [D.block(k, n, salt=i) for i, (k, n) in enumerate([(k, n) for k in ("json", "text", "zero") for n in (1, 13, 4096, 65536)])]
        d = D.dictionary("json")
        lay = layout(blocks, np.frombuffer(d, np.uint8), [7] * len(blocks), [0] * len(blocks))
        ref, _, st0 = run(dict(lay, out_buf=lay["out_buf"].copy()), mem, ext=False)
        assert (st0 == 0).all()
        for kw in ({"dict_base_null": True}, {}):
            outs, _, st = run(dict(lay, out_buf=lay["out_buf"].copy()), mem, **kw)
            assert outs == ref, kw
        mixed = dict(lay, out_buf=lay["out_buf"].copy(), dict_len=np.array([0, 4096] * (len(blocks) // 2), np.uint32))
        outs, _, st = run(mixed, mem)
        assert (st == 0).all()
        assert all(outs[i] == ref[i] for i in range(0, len(blocks), 2))
        decode_check(mixed, outs, st)
    finally:
        _mode("fast")


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("mem", ["host", "device"])
def test_refusals_and_small_outputs(mode, mem):
    """a dictionary with flags: INVALID_ARG, nothing written; out_cap below the maximum: OUTPUT_TOO_SMALL, nothing written; the other
    blocks of the batch are unaffected"""
    from lz4_flex_amd import _lib as L
    _mode(mode)
    try:
        d = D.dictionary("log")
        blocks = [D.block("log", 4096, salt=i) for i in range(8)]
        caps = [O.max_out(4096)] * 8
        caps[5] = O.max_out(4096) - 1
        lay = layout(blocks, np.frombuffer(d, np.uint8), [0] * 8, [len(d)] * 4 + [0, len(d), 0, 17], caps=caps)
        flags = [0, 2, 0, 1 << 8, 3, 0, 0, 3]
        outs, _, st = run(lay, mem, flags=flags)
        assert list(st) == [0, L.E_INVALID_ARG, 0, L.E_INVALID_ARG, 0, L.E_OUTPUT_TOO_SMALL, 0, L.E_INVALID_ARG], list(st)
        if mode == "fast":
            assert outs[0] == D.model(blocks[0], d) and outs[2] == D.model(blocks[2], d)
        else:
            assert outs[0] == O.compress_with_dict(blocks[0], d) and outs[6] == O.compress(blocks[6])
        decode_check(lay, outs, st)
    finally:
        _mode("fast")


def test_python_round_trips(fast):
    """compress_batch_with_dict (host) and compress_blocks_with_dict_device (torch) round-trip through decompress_batch_with_dict"""
    import torch
    from lz4_flex_amd import block
    d = D.dictionary("log")
    blocks = [D.block("log", n, salt=i) for i, n in enumerate([4096, 0, 1, 70000, 4096, 33])]
    src = np.frombuffer(b"".join(blocks), np.uint8)
    in_len = np.array([len(b) for b in blocks], np.uint32)
    in_off = np.cumsum([0] + list(in_len[:-1])).astype(np.uint64)
    doff = np.array([0, 0, 10, 0, 500000, 0], np.uint64)
    dlen = np.array([len(d), len(d), 100, 0, 40000, len(d)], np.uint32)
    dbuf = np.frombuffer(d, np.uint8)
    caps = np.array([O.max_out(int(n)) for n in in_len], np.uint32)
    ooff = np.cumsum([0] + list(caps[:-1])).astype(np.uint64)
    ob = np.zeros(int(caps.sum()), np.uint8)
    ol, st = block.compress_batch_with_dict(src, in_off, in_len, dbuf, doff, dlen, ob, ooff, caps)
    assert (st == 0).all()
    host = [bytes(ob[int(ooff[i]):int(ooff[i]) + int(ol[i])]) for i in range(len(blocks))]
    dev = torch.device("cuda")
    out, out_off, out_len, status = block.compress_blocks_with_dict_device(
        torch.from_numpy(src.copy()).to(dev), torch.from_numpy(in_off.view(np.int64)), torch.from_numpy(in_len.astype(np.int64)),
        torch.from_numpy(dbuf.copy()).to(dev), torch.from_numpy(doff.view(np.int64)), torch.from_numpy(dlen.astype(np.int64)))
    assert (status.cpu() == 0).all()
    o, oo, ln = out.cpu().numpy(), out_off.cpu().numpy(), out_len.cpu().numpy()
    devb = [bytes(o[int(oo[i]):int(oo[i]) + int(ln[i])]) for i in range(len(blocks))]
    assert devb == host                        # fast mode: the bytes never depend on the batch or the memory kind
    comp = np.frombuffer(b"".join(host) + b"\0", np.uint8)
    clen = np.array([len(x) for x in host], np.uint32)
    coff = np.cumsum([0] + list(clen[:-1])).astype(np.uint64)
    rt = np.zeros(int(in_len.sum()) + 1, np.uint8)
    rl, rs, _ = block.decompress_batch_with_dict(comp, coff, clen, dbuf, doff, dlen, rt, in_off, in_len)
    assert (rs == 0).all() and list(rl) == list(in_len)
    assert bytes(rt[:int(in_len.sum())]) == bytes(src)
