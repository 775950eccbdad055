"""GPU (-m gpu): which decoder each of the six batched decode entries takes under each setting, and what every block of a small batch
comes out as -- the routing table of lz4_route.h's decode_route (tests/test_host_routes.py holds it for the CPU), pinned from outside through the C ABI (MEM_DEVICE).

The six entries are the six forms of a batch: plain, one shared dictionary, a dictionary set, and each of those with partial targets.
Each gets one batch of at most six blocks of a few hundred bytes: a valid block with matches (the dictionary forms: one whose first
match starts inside the 17-byte dictionary, which lies at an address that is no multiple of 16), a damaged block whose offset reaches in
front of everything it may read, the valid block with a sink one byte too small (full forms) or with target 0 and a target inside a
match (partial forms), and for the sets a block without dictionary and one with an id the set does not have.

Expected values are the models': tests/oracle_api.py (the full forms), tests/partial_model.py and tests/partial_dict_model.py (the
partial forms).  FIRST_PASS is written by hand from the rule: a first-pass decoder runs unless "decompress_variant" is 1; a form with a
dictionary also needs "decompress_shared_dict" 1, a partial form also "decompress_partial" 1; the plain form asks for neither.
"decompress_second_pass" 0 makes the route visible: behind a first pass the damaged block (and the sink that is too small) stays marked
0x7F000001 with out_len 0, while the reference-order kernel marks nothing and gives the model's results alone."""
import ctypes as C

import numpy as np
import pytest

import oracle_api as O
import partial_dict_model as D
import partial_model as M
from lz4_writer import Writer

pytestmark = pytest.mark.gpu
REDO = 0x7F000001
INVALID = 64
NO_DICT = 0xFFFFFFFF
BAD_ID = 1                    # the set holds one dictionary
CANARY = 64
FILL = 0xA5
DICT_AT = CANARY + 3          # where the dictionary starts in its buffer: no multiple of 16
CODES = {"OutputTooSmall": 1, "LiteralOutOfBounds": 2, "ExpectedAnotherByte": 3, "OffsetZero": 4, "OffsetOutOfBounds": 5}

ENTRIES = ["plain", "shared_dict", "dict_set", "partial", "partial_shared_dict", "partial_dict_set"]
SETTINGS = ["decompress_variant", "decompress_shared_dict", "decompress_partial", "decompress_second_pass"]
ROWS = {"default": {}, "decompress_variant 1": {"decompress_variant": 1}, "decompress_shared_dict 0": {"decompress_shared_dict": 0},
        "decompress_partial 0": {"decompress_partial": 0}}
# 1: the entry's first-pass decoder runs (and the reference-order kernel behind it); 0: the reference-order kernel decodes every block
FIRST_PASS = {
    #                           plain  shared_dict  dict_set  partial  partial_shared_dict  partial_dict_set
    "default":                  (1,    1,           1,        1,       1,                   1),
    "decompress_variant 1":     (0,    0,           0,        0,       0,                   0),
    "decompress_shared_dict 0": (1,    0,           0,        1,       0,                   0),
    "decompress_partial 0":     (1,    1,           1,        0,       0,                   0),
}

DIC = D.dictionary(17)


def _blocks():
    """(plain block and its text, dictionary block and its text, damaged block, a target inside a match of each valid block)"""
    w = Writer(7)
    w.seq(70, 9, 8).seq(10, 66, 12).seq(3, 2, 30).seq(120, 40, 20)
    plain = w.end(5)
    w = Writer(8, prefix=DIC)
    w.seq(5, 14, 12)                    # the source starts 9 bytes in front of the dictionary's end: 9 bytes of it, 3 of the literals
    w.seq(70, 9, 8).seq(3, 2, 30).seq(120, 40, 20)
    with_dict = w.end(5)
    w = Writer(9, prefix=DIC)
    w.seq(20, 9, 8)
    w.bad_seq(6, 28 + 6 + len(DIC) + 1, 30)     # one byte in front of the dictionary's first (and far in front of a block without one)
    damaged = w.end(5)[0]
    return plain, with_dict, damaged, 74, 11


PLAIN, WITH_DICT, DAMAGED, PLAIN_CUT, DICT_CUT = _blocks()


def batch_of(entry):
    """[(name, block, cap or target, id)] of the entry's batch"""
    partial, has_dict, has_set = entry.startswith("partial"), entry != "plain" and entry != "partial", entry.endswith("dict_set")
    (c, p), cut = (WITH_DICT, DICT_CUT) if has_dict else (PLAIN, PLAIN_CUT)
    rows = [("valid", c, len(p), 0), ("damaged", DAMAGED, 300, 0)]
    if partial:
        rows += [("target 0", c, 0, 0), ("a target inside a match", c, cut, 0)]
    else:
        rows += [("a sink one byte too small", c, len(p) - 1, 0)]
    if has_set:
        rows += [("no dictionary", PLAIN[0], len(PLAIN[1]), NO_DICT), ("an id the set does not have", c, len(p), BAD_ID)]
    return rows


def model(entry, block, cap, dict_id):
    """(status, bytes, detail) -- detail None where the entry has none"""
    partial, has_dict = entry.startswith("partial"), entry != "plain" and entry != "partial"
    if dict_id == BAD_ID:
        return INVALID, b"", None if partial else (0, 0)
    dic = DIC if has_dict and dict_id != NO_DICT else None
    if partial:
        st, out = D.partial_with_dict(block, cap, dic) if dic else M.partial(block, cap)
        return st, out, None
    what, val = O.decompress(block, cap, dict_data=dic)
    if what == "ok":
        return 0, val, (0, 0)
    return CODES[what], b"", (val[0], cap) if what == "OutputTooSmall" else (0, 0)


def test_the_blocks_are_what_the_batches_need():
    assert 200 < len(PLAIN[1]) < 400 and 200 < len(WITH_DICT[1]) < 400 and len(DIC) == 17
    assert model("plain", PLAIN[0], len(PLAIN[1]), 0) == (0, PLAIN[1], (0, 0))
    assert model("shared_dict", WITH_DICT[0], len(WITH_DICT[1]), 0) == (0, WITH_DICT[1], (0, 0))
    assert O.decompress(WITH_DICT[0], len(WITH_DICT[1]))[0] == "OffsetOutOfBounds"          # (a match reaches into the dictionary)
    for entry in ENTRIES:
        assert model(entry, DAMAGED, 300, 0)[0] == 5, entry
    assert model("plain", PLAIN[0], len(PLAIN[1]) - 1, 0)[0] == 1 and model("shared_dict", WITH_DICT[0], len(WITH_DICT[1]) - 1, 0)[0] == 1
    assert M.partial(PLAIN[0], PLAIN_CUT) == (0, PLAIN[1][:PLAIN_CUT]) and 70 < PLAIN_CUT < 78
    assert D.partial_with_dict(WITH_DICT[0], DICT_CUT, DIC) == (0, WITH_DICT[1][:DICT_CUT]) and 5 < DICT_CUT < 14
    assert set(FIRST_PASS) == set(ROWS) and all(len(v) == len(ENTRIES) for v in FIRST_PASS.values())
    assert all(len(batch_of(e)) <= 6 for e in ENTRIES)


@pytest.fixture(scope="module")
def env():
    import torch
    from lz4_flex_amd import _lib
    lib = _lib.load()
    assert lib.lz4flex_device_count() >= 1, _lib.last_error()
    ctx, h = C.c_void_p(), C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
    defaults = {k: lib.lz4flex_get_tuning(ctx, k.encode()) for k in SETTINGS}
    assert defaults == {"decompress_variant": 0, "decompress_shared_dict": 1, "decompress_partial": 1, "decompress_second_pass": 1}, defaults
    flat = np.frombuffer(DIC + b"\0", dtype=np.uint8).copy()
    offs, lens = np.zeros(1, dtype=np.uint64), np.array([len(DIC)], dtype=np.uint32)
    rc = lib.lz4flex_dict_set_create(ctx, C.c_void_p(flat.ctypes.data), C.c_void_p(offs.ctypes.data), C.c_void_p(lens.ctypes.data), 1, _lib.MEM_HOST,
                                     C.byref(h))
    assert rc == 0 and h.value, (rc, _lib.last_error())
    yield lib, _lib, torch, ctx, h, defaults
    torch.cuda.synchronize()
    lib.lz4flex_dict_set_free(h)
    lib.lz4flex_ctx_destroy(ctx)


def run(env, entry, rows):
    """the entry's call on device memory: (sinks' buffer, out_off, out_len, status, detail or None)"""
    lib, L, torch, ctx, h = env[:5]
    n = len(rows)
    partial = entry.startswith("partial")
    comps = [r[1] for r in rows]
    in_len = np.array([len(c) for c in comps], dtype=np.uint32)
    in_off = (np.concatenate([[0], np.cumsum(in_len[:-1], dtype=np.uint64)]) + 3).astype(np.uint64)
    inb = np.frombuffer(bytes(3) + b"".join(comps) + bytes(64), dtype=np.uint8).copy()
    cap = np.array([r[2] for r in rows], dtype=np.uint32)
    off, o = [], 0
    for r in rows:
        o += CANARY
        if o % 16 == 0:
            o += 5
        off.append(o)
        o += r[2] + CANARY
    out_off = np.array(off, dtype=np.uint64)
    dbuf = np.frombuffer(bytes([FILL]) * DICT_AT + DIC + bytes([FILL]) * CANARY, dtype=np.uint8).copy()
    arrays = dict(inb=inb, in_off=in_off, in_len=in_len, out=np.full(o + 64, FILL, dtype=np.uint8), out_off=out_off, cap=cap,
                  out_len=np.full(n, 0xDEADBEEF, dtype=np.uint32), status=np.full(n, -1, dtype=np.int32),
                  detail=np.full((n, 2), 0xEE, dtype=np.uint64), dbuf=dbuf.copy(), ids=np.array([r[3] for r in rows], dtype=np.uint32))
    dev = torch.device("cuda", 0)
    keep = {k: torch.from_numpy(v.view(np.uint8).reshape(-1)).to(dev) for k, v in arrays.items()}
    p = {k: C.c_void_p(v.data_ptr()) for k, v in keep.items()}
    assert (keep["dbuf"].data_ptr() + DICT_AT) % 16 != 0
    dp, dn = C.c_void_p(keep["dbuf"].data_ptr() + DICT_AT), len(DIC)
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    head = (ctx, p["inb"], p["in_off"], p["in_len"], n)
    sink = (p["out"], p["out_off"], p["cap"], p["out_len"], p["status"])
    mem = L.MEM_DEVICE
    if entry == "plain":
        rc = lib.lz4flex_decompress_batch(*head, *sink, p["detail"], mem, sp)
    elif entry == "shared_dict":
        rc = lib.lz4flex_decompress_batch_shared_dict(*head, *sink, p["detail"], dp, dn, mem, sp)
    elif entry == "dict_set":
        rc = lib.lz4flex_decompress_batch_dict_set(*head, p["ids"], *sink, p["detail"], h, mem, sp)
    elif entry == "partial":
        rc = lib.lz4flex_decompress_batch_partial(*head, *sink, mem, sp)
    elif entry == "partial_shared_dict":
        rc = lib.lz4flex_decompress_batch_partial_shared_dict(*head, *sink, dp, dn, mem, sp)
    else:
        rc = lib.lz4flex_decompress_batch_partial_dict_set(*head, p["ids"], *sink, h, mem, sp)
    assert rc == 0, (entry, rc, L.last_error())
    torch.cuda.synchronize()
    for k in ("inb", "out", "out_len", "status", "detail", "dbuf"):
        arrays[k].view(np.uint8).reshape(-1)[:] = keep[k].cpu().numpy()
    assert np.array_equal(arrays["inb"], inb), "the input buffer was written"
    assert np.array_equal(arrays["dbuf"], dbuf), "the dictionary or the bytes around it were written"
    return arrays["out"], out_off, arrays["out_len"], arrays["status"], None if partial else arrays["detail"]


@pytest.mark.parametrize("second_pass", [1, 0])
@pytest.mark.parametrize("row", list(ROWS))
@pytest.mark.parametrize("entry", ENTRIES)
def test_route(env, entry, row, second_pass):
    lib, ctx, defaults = env[0], env[3], env[5]
    first_pass = FIRST_PASS[row][ENTRIES.index(entry)]
    rows = batch_of(entry)
    want = [model(entry, c, cap, i) for _, c, cap, i in rows]
    tuning = dict(defaults, **ROWS[row], decompress_second_pass=second_pass)
    try:
        for k, v in tuning.items():
            assert lib.lz4flex_set_tuning(ctx, k.encode(), v) == 0, k
        out, out_off, out_len, status, detail = run(env, entry, rows)
    finally:
        for k, v in defaults.items():
            assert lib.lz4flex_set_tuning(ctx, k.encode(), v) == 0, k
    what = (entry, row, "second pass %d" % second_pass)
    print(what, [hex(int(s)) for s in status], out_len.tolist(), None if detail is None else detail.tolist())
    exp = np.full(len(out), FILL, dtype=np.uint8)
    care = np.ones(len(out), dtype=bool)
    for i, ((name, _c, cap, _id), (wst, wbytes, wdet)) in enumerate(zip(rows, want)):
        st, ol, o = int(status[i]), int(out_len[i]), int(out_off[i])
        if wst != INVALID:
            care[o:o + cap] = False                             # (a failed block may have written part of its sink; a refused one has not)
        if not second_pass and first_pass and wst not in (0, INVALID):
            assert (st, ol) == (REDO, 0), (what, name, hex(st), ol)         # left to a second pass that does not run
            continue
        assert st != REDO and (st, ol) == (wst, len(wbytes)), (what, name, hex(st), ol, wst, len(wbytes))
        # (the plain entry's header promises the words for OutputTooSmall alone, and its workgroup decoder leaves a decoded block's as
        # they were; the dictionary entries zero them, which tests/test_gpu_decompress_shared_dict.py asserts too)
        if detail is not None and not (entry == "plain" and wst == 0):
            assert tuple(int(v) for v in detail[i]) == wdet, (what, name, detail[i].tolist(), wdet)
        if st == 0:
            exp[o:o + ol] = np.frombuffer(wbytes, dtype=np.uint8)
            care[o:o + ol] = True
    bad = np.nonzero((out != exp) & care)[0]
    assert len(bad) == 0, (what, "%d wrong bytes, the first at %d" % (len(bad), int(bad[0])), out_off.tolist())
    if not second_pass and first_pass:
        assert REDO in set(int(s) for s in status), what        # (the damaged block shows that a first pass ran)
