"""GPU: lz4flex_compress_batch_shared_dict -- a batch compressed against ONE dictionary whose digest (the indexer's table after the
dictionary's tail) is built once per call.

The contract is bytes: block i gets what lz4flex_compress_batch_ex gives it with that dictionary -- in fast mode the scalar model's
lz4w_compress(dict[-h:] + block, hist = h) (tests/dict_cases.py), in exact mode the oracle's compress_into_with_dict.  Equal bytes
cannot show that the digest was used, so every fast-mode call also reads the context's counter of items whose first window started
from the digest and compares it with the number the eligibility rule gives."""
import ctypes as C

import numpy as np
import pytest

import dict_cases as D
import oracle_api as O
import wave_model as W

pytestmark = pytest.mark.gpu

CANARY = 0xA5
PAD = 64
CHUNK = 1024
# dictionary lengths: those of the per-block tests, the digest's own edges (hs = the largest multiple of 1 024 with hs + 3 <= h: the first
# h with a digest is 1 027; 31 744 + 3 is the first with the full 31 chunks ... ) and dictionaries longer than 32 KiB, whose tail alone counts
DICT_LENS = D.HS + [1023, 1024, 1026, 1027, 1028, 2047, 2051, 31744 + 2, 31744 + 3, 31744 + 4, 40000, D.DICT_BYTES]
# block lengths: the per-block tests', the eligibility edge (a block of 11 - (h - hs) bytes or more: 8 for h = hs + 3), a record either
# side of 4 KiB and of a half window, a block of several windows
BLOCK_LENS = D.LENS + [2, 7, 8, 11, 4095, 4097, 32767, 32769]


def _L():
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
    assert _L().load().lz4flex_set_tuning(None, key.encode(), v) == 0


def counter():
    v = _L().load().lz4flex_get_tuning(None, b"debug_shared_dict_items")
    assert v >= 0, v
    return v


def hs_of(dict_len):
    h = min(dict_len, W.HIST)
    return (h - 3) // CHUNK * CHUNK if h >= CHUNK + 3 else 0


def eligible(dict_len, block_len, cap=None):
    """the rule of the header: the item [h | block] starts from the digest when there is one (hs > 0), the block is encoded at all
    (out_cap at least the maximum output size) and every position below hs may start a match (positions < item length - 11 do)"""
    h = min(dict_len, W.HIST)
    hs = hs_of(dict_len)
    if cap is not None and cap < O.max_out(block_len):
        return False
    n = h + block_len
    active = n - 11 if n >= 12 else 0
    return hs > 0 and min(active, n, 65536) >= hs


def layout(blocks, caps=None, odd=True):
    in_off, pos = [], 1 if odd else 0
    for b in blocks:
        in_off.append(pos)
        pos += len(b) + (3 if odd else 0)
    in_buf = np.full(pos + PAD, CANARY, np.uint8)
    for o, b in zip(in_off, blocks):
        in_buf[o:o + len(b)] = np.frombuffer(b, np.uint8)
    caps = [O.max_out(len(b)) for b in blocks] if caps is None else caps
    out_off, pos = [], 5 if odd else 0
    for c in caps:
        out_off.append(pos)
        pos += c + PAD
    return dict(in_buf=in_buf, in_off=np.array(in_off, np.uint64), in_len=np.array([len(b) for b in blocks], np.uint32),
                out_buf=np.full(pos, CANARY, np.uint8), out_off=np.array(out_off, np.uint64), out_cap=np.array(caps, np.uint32))


def _dev(a):
    import torch
    v = a.view(np.int64) if a.dtype == np.uint64 else (a.view(np.int32) if a.dtype == np.uint32 else a)
    return torch.from_numpy(v.copy()).to("cuda")


def run(lay, d, mem="host", entry="shared", dict_null=False):
    """one call of the shared entry (or of lz4flex_compress_batch_ex with the same dictionary for every block); returns (outputs,
    status); checks the canaries behind every output slot, behind the inputs and around the dictionary"""
    import torch
    L = _L()
    lib = L.load()
    n = len(lay["in_off"])
    dbuf = np.full(len(d) + 2 * PAD + 3, CANARY, np.uint8)           # the dictionary at an odd address between canaries
    d0 = PAD + 3
    dbuf[d0:d0 + len(d)] = np.frombuffer(d, np.uint8)
    dict_off = np.full(n, d0, np.uint64)
    dict_len = np.full(n, len(d), np.uint32)
    out_buf = lay["out_buf"].copy()
    if mem == "host":
        p = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731
        in_buf = lay["in_buf"].copy()
        out_len = np.zeros(n, np.uint32)
        status = np.full(n, -1, np.int32)
        if entry == "shared":
            rc = lib.lz4flex_compress_batch_shared_dict(None, p(in_buf), p(lay["in_off"]), p(lay["in_len"]), n, p(out_buf), p(lay["out_off"]),
                                                        p(lay["out_cap"]), p(out_len), p(status),
                                                        None if dict_null else C.c_void_p(dbuf.ctypes.data + d0), len(d), L.MEM_HOST, None)
        else:
            e = L.CompressExt(dbuf.ctypes.data, dict_off.ctypes.data, dict_len.ctypes.data)
            rc = lib.lz4flex_compress_batch_ex(None, p(in_buf), p(lay["in_off"]), p(lay["in_len"]), None, n, p(out_buf), p(lay["out_off"]),
                                               p(lay["out_cap"]), p(out_len), p(status), C.byref(e), L.MEM_HOST, None)
        assert rc == 0, (rc, L.last_error())
        in_after, d_after = in_buf, dbuf
    else:
        t = {k: _dev(v) for k, v in lay.items()}
        t["out_buf"] = _dev(out_buf)
        td, tdo, tdl = _dev(dbuf), _dev(dict_off), _dev(dict_len)
        out_len = torch.zeros(n, dtype=torch.int32, device="cuda")
        status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        q = lambda x: C.c_void_p(x.data_ptr())        # noqa: E731
        big = L.MEM_BIG_BLOCKS if int(lay["in_len"].max(initial=0)) > 65536 else 0
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if entry == "shared":
            rc = lib.lz4flex_compress_batch_shared_dict(None, q(t["in_buf"]), q(t["in_off"]), q(t["in_len"]), n, q(t["out_buf"]), q(t["out_off"]),
                                                        q(t["out_cap"]), q(out_len), q(status),
                                                        None if dict_null else C.c_void_p(td.data_ptr() + d0), len(d), L.MEM_DEVICE | big, s)
        else:
            e = L.CompressExt(td.data_ptr(), tdo.data_ptr(), tdl.data_ptr())
            rc = lib.lz4flex_compress_batch_ex(None, q(t["in_buf"]), q(t["in_off"]), q(t["in_len"]), None, n, q(t["out_buf"]), q(t["out_off"]),
                                               q(t["out_cap"]), q(out_len), q(status), C.byref(e), L.MEM_DEVICE | big, s)
        assert rc == 0, (rc, L.last_error())
        torch.cuda.synchronize()
        out_buf = t["out_buf"].cpu().numpy()
        out_len = out_len.cpu().numpy().view(np.uint32)
        status = status.cpu().numpy()
        in_after, d_after = t["in_buf"].cpu().numpy(), td.cpu().numpy()
    assert (in_after == lay["in_buf"]).all(), "the input (or the canary behind it) was written"
    assert (d_after == dbuf).all(), "the dictionary (or a canary around it) was written"
    outs = []
    first = int(lay["out_off"][0]) if n else 0
    assert (out_buf[:first] == CANARY).all()
    for i in range(n):
        o, c, m = int(lay["out_off"][i]), int(lay["out_cap"][i]), int(out_len[i])
        if status[i] != 0:
            assert m == 0
            assert (out_buf[o:o + c + PAD] == CANARY).all(), "block %d (status %d) wrote bytes" % (i, status[i])
        else:
            assert (out_buf[o + m:o + c + PAD] == CANARY).all(), "block %d wrote behind its length" % i
        outs.append(bytes(out_buf[o:o + m]))
    return outs, status


def decode_check(blocks, outs, status, d, oracle_every=5):
    """every good block decodes with lz4flex_decompress_batch_ex and the dictionary to its input; the oracle decodes a sample"""
    from lz4_flex_amd import block
    good = [i for i in range(len(outs)) if status[i] == 0]
    for i in good[::oracle_every]:
        assert D.oracle_decodes(outs[i], blocks[i], d), i
    if not good:
        return
    comp = np.frombuffer(b"".join(outs[i] for i in good) + b"\0", np.uint8)
    clen = np.array([len(outs[i]) for i in good], np.uint32)
    coff = (np.cumsum(clen, dtype=np.uint64) - clen).astype(np.uint64)
    ocap = np.array([len(blocks[i]) for i in good], np.uint32)
    ooff = (np.cumsum(ocap, dtype=np.uint64) - ocap).astype(np.uint64)
    out = np.zeros(int(ocap.sum()) + 1, np.uint8)
    db = np.frombuffer(d, np.uint8) if len(d) else np.zeros(1, np.uint8)
    ol, st, _ = block.decompress_batch_with_dict(comp, coff, clen, db, np.zeros(len(good), np.uint64), np.full(len(good), len(d), np.uint32),
                                                 out, ooff, ocap)
    assert (st == 0).all(), st
    for k, i in enumerate(good):
        assert int(ol[k]) == len(blocks[i]) and bytes(out[int(ooff[k]):int(ooff[k]) + len(blocks[i])]) == blocks[i], i


def dict_of(kind, n):
    full = D.dictionary(kind)
    return full if n == len(full) else full[len(full) - n:]


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("kind", D.KINDS)
def test_fast_equals_model(fast, kind, mem):
    """every dictionary length x every block length of a kind (one call per dictionary: window mode, the carry ring for the long
    blocks): the model's bytes, the round trip, and the digest counter"""
    for k, dl in enumerate(DICT_LENS):
        d = dict_of(kind, dl)
        blocks = [D.block(kind, n, salt=(k + j) % 7) for j, n in enumerate(BLOCK_LENS)]
        lay = layout(blocks)
        outs, st = run(lay, d, mem)
        assert (st == 0).all(), (dl, st)
        assert counter() == sum(eligible(dl, len(b)) for b in blocks), dl
        bad = [(dl, len(b)) for b, o in zip(blocks, outs) if o != D.model(b, d)]
        assert not bad, bad[:8]
        decode_check(blocks, outs, st, d)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_run_windows(fast, mem):
    """a zero dictionary with a non-zero block, the reverse, and zeros on zeros (the digest says "one byte repeated": the run-window test
    must decide as the per-block path does); a dictionary of another repeated byte in front of zeros"""
    z = bytes(40000)
    for d, kinds in ((z, ("json", "zero", "log")), (D.dictionary("json")[-40000:], ("zero",)), (b"\x07" * 40000, ("zero",)),
                     (z[:5000], ("zero", "text"))):
        blocks = [D.block(k, n, salt=3) for k in kinds for n in (11, 4096, 8192, 32769, 65536, 200000)]
        lay = layout(blocks)
        outs, st = run(lay, d, mem)
        assert (st == 0).all()
        assert counter() == sum(eligible(len(d), len(b)) for b in blocks)
        bad = [i for i, (b, o) in enumerate(zip(blocks, outs)) if o != D.model(b, d)]
        assert not bad, bad
        decode_check(blocks, outs, st, d, oracle_every=1)


def mixed_batch(n):
    lens = [4096, 1, 12, 13, 700, 65536, 20000, 0, 2, 7, 8, 11, 4095, 4097, 40000]
    return [D.block("log", lens[i % len(lens)], salt=i) for i in range(n)]


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("dict_len", [40000, 1027 + 4, 3])
def test_block_mode_thousands_of_blocks(fast, mem, dict_len):
    """2 304 blocks at odd offsets (more blocks than workgroups: block mode, a workgroup goes from item to item and keeps the staged tail),
    eligible and ineligible items mixed, some too small an output: the bytes of lz4flex_compress_batch_ex and of the entry with
    "compress_shared_dict" 0, the model's on a sample; the counter is the number of eligible items, 0 with the setting off and 0 for
    a 3-byte dictionary"""
    L = _L()
    d = D.stream("log", dict_len, 5_000_000)
    blocks = mixed_batch(2304)
    caps = [O.max_out(len(b)) - (1 if i % 97 == 5 else 0) for i, b in enumerate(blocks)]
    lay = layout(blocks, caps=caps)
    outs, st = run(lay, d, mem)
    want_el = sum(eligible(dict_len, len(b), c) for b, c in zip(blocks, caps))
    assert counter() == want_el
    if dict_len == 3:
        assert want_el == 0
    else:
        assert want_el > 1500
    small = [i for i in range(len(blocks)) if i % 97 == 5]
    assert all(st[i] == L.E_OUTPUT_TOO_SMALL for i in small) and all(st[i] == 0 for i in range(len(blocks)) if i % 97 != 5)
    ref, st_ref = run(lay, d, mem, entry="ex")
    assert list(st_ref) == list(st)
    assert outs == ref
    _tuning("compress_shared_dict", 0)
    try:
        off, st_off = run(lay, d, mem)
        assert counter() == 0
    finally:
        _tuning("compress_shared_dict", 1)
    assert list(st_off) == list(st) and off == ref
    for i in range(0, len(blocks), 7):
        if st[i] == 0:
            assert outs[i] == D.model(blocks[i], d), i
    decode_check(blocks, outs, st, d, oracle_every=50)


@pytest.mark.parametrize("carry_wait", [1, 0])
@pytest.mark.parametrize("kind", ["json", "log"])
def test_window_mode_large_blocks(fast, kind, carry_wait):
    """1 - 3 large blocks: the windows of an item are drawn by different workgroups (the carry ring); with "compress_carry_wait" 0 a window
    that would wait gives up and the redo launch encodes its block again -- the counter counts an item once"""
    _tuning("compress_carry_wait", carry_wait)
    try:
        for lens, dl in (([1 << 20], 32768), ([300001, 1 << 20], 40000), ([1 << 20, 65537, 300001], 2051), ([500000], 513)):
            d = dict_of(kind, dl)
            blocks = [D.block(kind, n, salt=j) for j, n in enumerate(lens)]
            lay = layout(blocks)
            outs, st = run(lay, d, "device")
            assert (st == 0).all(), st
            assert counter() == sum(eligible(dl, len(b)) for b in blocks)
            for b, o in zip(blocks, outs):
                assert o == D.model(b, d), (dl, len(b))
            decode_check(blocks, outs, st, d, oracle_every=1)
    finally:
        _tuning("compress_carry_wait", 1)


@pytest.mark.parametrize("sliding", [0, 1, 2])
def test_every_sliding_window_setting(fast, sliding):
    """the bytes of lz4flex_compress_batch_ex under every "compress_sliding_window" (an item with history always advances by 32 KiB: the
    model's bytes too)"""
    _tuning("compress_sliding_window", sliding)
    try:
        d = dict_of("text", 40000)
        blocks = [D.block("text", n, salt=j) for j, n in enumerate([4096, 65536, 65537, 200000, 11])]
        lay = layout(blocks)
        for mem in ("host", "device"):
            outs, st = run(lay, d, mem)
            ref, _ = run(lay, d, mem, entry="ex")
            assert (st == 0).all() and outs == ref
            assert outs == [D.model(b, d) for b in blocks]
    finally:
        _tuning("compress_sliding_window", 2)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_exact_equals_oracle(exact, mem):
    """compress_mode exact: the oracle's compress_into_with_dict, both sides of the table-kind boundary; the digest is not involved"""
    full = D.dictionary("json")
    for k in (1, 3, 4, 100, 1000, 65536, 65537, 1 << 20):
        d = full[len(full) - k:]
        lens = [4096, 0, 13, 65530, 300000, 64534, 64535]
        blocks = [D.block("json", n, salt=j) for j, n in enumerate(lens)]
        caps = [O.max_out(n) for n in lens]
        caps[2] -= 1
        lay = layout(blocks, caps=caps)
        outs, st = run(lay, d, mem)
        assert [int(x) for x in st] == [0, 0, _L().E_OUTPUT_TOO_SMALL, 0, 0, 0, 0], st
        assert counter() == 0
        for j, b in enumerate(blocks):
            if st[j] == 0:
                assert outs[j] == O.compress_with_dict(b, d), (k, len(b))
        ref, st_ref = run(lay, d, mem, entry="ex")
        assert outs == ref and list(st) == list(st_ref)
        decode_check(blocks, outs, st, d, oracle_every=1)


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("mem", ["host", "device"])
def test_no_dictionary_is_the_plain_batch(mode, mem):
    """dict_len == 0 or dict == NULL: lz4flex_compress_batch without flags"""
    from lz4_flex_amd import block
    _mode(mode)
    try:
        blocks = [D.block(k, n, salt=i) for i, (k, n) in enumerate([(k, n) for k in ("json", "zero") for n in (1, 13, 4096, 65536)])]
        lay = layout(blocks, odd=False)
        a, st_a = run(lay, b"", mem)
        b, st_b = run(lay, b"", mem, dict_null=True)
        assert (st_a == 0).all() and (st_b == 0).all() and a == b
        ol = np.zeros(len(blocks), np.uint32)
        ob = lay["out_buf"].copy()
        ol, st = block.compress_batch(lay["in_buf"], lay["in_off"], lay["in_len"], ob, lay["out_off"], lay["out_cap"])
        assert (st == 0).all()
        assert a == [bytes(ob[int(o):int(o) + int(m)]) for o, m in zip(lay["out_off"], ol)]
    finally:
        _mode("fast")


def test_context_reuse_back_to_back(fast):
    """two calls with different dictionaries on one context and one stream without a synchronisation between them (the second digest
    overwrites the first once the first encoder is done), then a plain lz4flex_compress_batch: each its own model's bytes"""
    import torch
    L = _L()
    lib = L.load()
    blocks = mixed_batch(1200)
    lay = layout(blocks, odd=True)
    d1, d2 = D.stream("log", 40000, 5_000_000), D.stream("log", 32768, 9_000_000)
    t = {k: _dev(v) for k, v in lay.items()}
    q = lambda x: C.c_void_p(x.data_ptr())        # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = []
    n = len(blocks)
    td = [_dev(np.frombuffer(d, np.uint8)) for d in (d1, d2)]
    for k in range(3):
        ob = _dev(lay["out_buf"])
        ol = torch.zeros(n, dtype=torch.int32, device="cuda")
        stt = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        if k < 2:
            rc = lib.lz4flex_compress_batch_shared_dict(None, q(t["in_buf"]), q(t["in_off"]), q(t["in_len"]), n, q(ob), q(t["out_off"]),
                                                        q(t["out_cap"]), q(ol), q(stt), q(td[k]), td[k].numel(), L.MEM_DEVICE, s)
        else:
            rc = lib.lz4flex_compress_batch(None, q(t["in_buf"]), q(t["in_off"]), q(t["in_len"]), None, n, q(ob), q(t["out_off"]),
                                            q(t["out_cap"]), q(ol), q(stt), L.MEM_DEVICE, s)
        assert rc == 0, (rc, L.last_error())
        res.append((ob, ol, stt))
    torch.cuda.synchronize()
    wgs = lib.lz4flex_get_tuning(None, b"compress_workgroups")
    for k, (ob, ol, stt) in enumerate(res):
        assert int((stt != 0).sum()) == 0
        o, m = ob.cpu().numpy(), ol.cpu().numpy()
        for i in range(0, n, 5):
            if k == 2 and not len(blocks[i]):
                continue
            got = bytes(o[int(lay["out_off"][i]):int(lay["out_off"][i]) + int(m[i])])
            want = D.model(blocks[i], (d1, d2)[k]) if k < 2 else W.compress(blocks[i], sub=W.auto_sub(n, wgs))
            assert got == want, (k, i, len(blocks[i]))


def test_python_wrappers_round_trip(fast):
    import torch
    from lz4_flex_amd import block
    d = D.dictionary("log")
    blocks = [D.block("log", n, salt=i) for i, n in enumerate([4096, 0, 1, 70000, 4096, 33])]
    src = np.frombuffer(b"".join(blocks), np.uint8)
    in_len = np.array([len(b) for b in blocks], np.uint32)
    in_off = (np.cumsum(in_len, dtype=np.uint64) - in_len).astype(np.uint64)
    caps = np.array([O.max_out(int(n)) for n in in_len], np.uint32)
    ooff = (np.cumsum(caps, dtype=np.uint64) - caps).astype(np.uint64)
    ob = np.zeros(int(caps.sum()), np.uint8)
    ol, st = block.compress_batch_with_shared_dict(src, in_off, in_len, d, ob, ooff, caps)
    assert (st == 0).all()
    host = [bytes(ob[int(ooff[i]):int(ooff[i]) + int(ol[i])]) for i in range(len(blocks))]
    assert host == [D.model(b, d) for b in blocks]
    out, out_off, out_len, status = block.compress_blocks_with_shared_dict_device(
        torch.from_numpy(src.copy()).to("cuda"), torch.from_numpy(in_off.view(np.int64)), torch.from_numpy(in_len.astype(np.int64)),
        torch.from_numpy(np.frombuffer(d, np.uint8).copy()).to("cuda"))
    assert (status.cpu() == 0).all()
    o, oo, ln = out.cpu().numpy(), out_off.cpu().numpy(), out_len.cpu().numpy()
    assert [bytes(o[int(oo[i]):int(oo[i]) + int(ln[i])]) for i in range(len(blocks))] == host
    decode_check(blocks, host, st, d, oracle_every=1)
