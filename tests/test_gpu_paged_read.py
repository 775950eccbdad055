"""GPU tests of lz4flex_paged_read_ranges (lz4_paged_read.hip, paged_range.h): m byte ranges of paged streams in one call, MEM_HOST and
MEM_DEVICE.  The tables come from the existing block.compress_paged; the expected out_len / status of every range come from
tests/paged_read_model.py; the expected BYTES are the source's own (`src_i[off : off + out_len]`) -- no decoder of this library takes
part in them.  Only where a page is damaged or a table is hostile does the expectation of the ranges that touch it come from
lz4flex_decompress_batch_partial on those pages alone (an entry of its own, with its own tests), folded by the model.

In MEM_DEVICE every range's region sits between canaries in a filled buffer and the tables and the page file are compared before and
after: nothing but the regions' first out_len bytes, out_len and status changes."""
import ctypes as C

import numpy as np
import pytest

import paged_cases as K
import paged_read_model as R

pytestmark = pytest.mark.gpu

FILL, GAP, FIRST = 0xC5, 9, 2
CUT = {64: 4096, 509: 20 * 1024, 4096: 20 * 1024}
SETS = ["n37@64", "n37@509", "n37@4096", "json@64", "noise@64", "zeros@64", "len0@64", "len13@64", "short@64"]
CLASSES = ("zero:at_end", "zero:behind_end", "zero:len0", "page_start", "head_one_page", "ends_at_page_end", "three_pages_head_tail", "whole",
           "last_byte", "no_pages", "big_head", "no_stream")
STRICT = (0, R.E_OUTPUT_TOO_SMALL, R.E_INVALID_ARG)      # statuses under which nothing but [0, out_len) of the region may change


@pytest.fixture(scope="module")
def lib():
    from lz4_flex_amd import _lib
    lib = _lib.load()
    if lib.lz4flex_device_count() < 1:
        pytest.fail("GPU tests need a device: " + _lib.last_error())
    return lib


class Set:
    """one batch of paged streams: the sources, the tables as the entry takes them (entries from FIRST on: two pages of filler lie in
    front of the page file) and as the model takes them"""

    def __init__(self, data, P, page_cap=None):
        from lz4_flex_amd import block
        block.set_compress_mode("fast")
        res = block.compress_paged(data, P, page_cap=page_cap)
        self.data, self.P = data, P
        self.arrays = dict(pages=np.concatenate([np.full(FIRST * P, 0x77, np.uint8), res.pages]), page_off=res.page_off + np.uint64(FIRST),
                           page_len=np.concatenate([np.full(FIRST, 0x5A5A5A5A, np.uint32), res.page_len]),
                           page_src=np.concatenate([np.full(FIRST, 0x5A5A5A5A, np.uint32), res.page_src]), n_pages=res.n_pages.copy(),
                           in_done=res.in_done.copy())
        self.status = res.status

    @property
    def t(self):
        return model_of(self.arrays, self.P)


def model_of(arrays, P):
    return R.Tables(P, arrays["page_off"], arrays["page_len"], arrays["page_src"], arrays["n_pages"], arrays["in_done"])


_sets = {}


def the_set(name):
    if name not in _sets:
        which, P = name.split("@")
        P = int(P)
        cases = K.streams(P, cut=CUT[P])
        if which == "n37":
            _sets[name] = Set([cases[(5 * j) % len(cases)][1] for j in range(37)], P)
        elif which == "short":                         # out of pages after 5: OUTPUT_TOO_SMALL, valid pages so far, in_done < in_len
            _sets[name] = Set([dict(cases)["json"]], P, page_cap=[5])
        else:
            _sets[name] = Set([dict(cases)[which]], P)
    return _sets[name]


def ranges_of(t):
    """[(stream, off, len)] computed from the tables, and the classes they fall into by the model: {class: count}"""
    out = []
    for i in range(t.n):
        S, first, k = t.in_done[i], t.page_off[i], t.n_pages[i]
        src = t.page_src[first:first + k] + [S]
        out += [(i, S, 5), (i, S + 3, 5), (i, 0, 0), (i, 0, R.WHOLE), (i, 0, 1)]
        if S:
            out.append((i, S - 1, 1))
        for j in sorted({0, k // 2, k - 1} & set(range(k))):
            size = src[j + 1] - src[j]
            out.append((i, src[j], min(10, size)))
            if size >= 3:
                out += [(i, src[j] + 1, size - 2), (i, src[j] + size // 2, size - size // 2)]
            if j + 3 <= k:
                out.append((i, src[j] + 1, src[j + 2] + 1 - (src[j] + 1)))
        if S >= 4096 and k and src[1] >= 4096:         # a page that decodes to several KiB: a large head slot
            out.append((i, 1000, 3000))
    out.append((t.n, 0, 7))
    count = dict.fromkeys(CLASSES, 0)
    for i, off, length in out:
        rec = R.locate(t, i, off, length)
        if rec.no_stream:
            count["no_stream"] += 1
            continue
        if t.n_pages[i] == 0:
            count["no_pages"] += 1
        if rec.len == 0:
            count["zero:len0" if length == 0 else "zero:at_end" if off == rec.S else "zero:behind_end"] += 1
            continue
        end_page = t.page_src[rec.first + rec.j0 + rec.nb] if rec.j0 + rec.nb < rec.k else rec.S
        count["page_start"] += rec.nb == 1 and not rec.head
        count["head_one_page"] += rec.nb == 1 and rec.head
        count["ends_at_page_end"] += off + rec.len == end_page
        count["three_pages_head_tail"] += rec.nb >= 3 and rec.head and off + rec.len < end_page
        count["whole"] += length == R.WHOLE and off == 0
        count["last_byte"] += off == rec.S - 1 and rec.len == 1
        count["big_head"] += rec.head and rec.head_bytes >= 2048
    return out, count


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else C.c_void_p(a.data_ptr())


def _dev(a):
    import torch
    v = a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a
    return torch.from_numpy(np.array(v)).to(torch.device("cuda", 0))


TABLES = ("pages", "page_off", "page_len", "page_src", "n_pages", "in_done")


def run_read(lib, arrays, P, ranges, mem, max_items, scratch_cap):
    """one lz4flex_paged_read_ranges.  Returns (status, out_len, bytes per range) after checking that nothing but the regions' bytes the
    statuses allow, out_len and status was written"""
    from lz4_flex_amd import _lib
    m, n = len(ranges), len(arrays["n_pages"])
    sid, off, length = (np.array([r[k] for r in ranges], np.uint32) for k in range(3))
    room = [min(ln, int(arrays["in_done"][i]) - o) if i < n and o < int(arrays["in_done"][i]) else 0 for i, o, ln in ranges]
    out_off = np.zeros(m, np.uint64)
    at = GAP
    for r in range(m):
        out_off[r] = at
        at += room[r] + GAP
    out = np.full(at + 64, FILL, np.uint8)
    out_len, status = np.full(m + 3, 0x5A5A5A5A, np.uint32), np.full(m + 3, 0x5A5A5A5A, np.int32)
    tables = [arrays[k] if arrays[k].size else np.zeros(1, arrays[k].dtype) for k in TABLES]
    before = [a.copy() for a in tables]
    if mem == "host":
        p = [_ptr(a) for a in tables]
        rc = lib.lz4flex_paged_read_ranges(None, p[0], P, *p[1:], n, _ptr(sid), _ptr(off), _ptr(length), m, _ptr(out), _ptr(out_off), _ptr(out_len),
                                           _ptr(status), 0, None, 0, None, _lib.MEM_HOST, None)
        assert rc == 0, _lib.last_error()
        after = tables
    else:
        import torch
        d = [_dev(a) for a in tables + [sid, off, length, out, out_off, out_len, status]]
        scratch = torch.full((scratch_cap + 64,), 0x11, dtype=torch.uint8, device=d[0].device)
        work = torch.empty(int(lib.lz4flex_paged_read_work_size(m, max_items)), dtype=torch.uint8, device=d[0].device)
        stream = torch.cuda.current_stream(d[0].device)
        p = [_ptr(x) for x in d]
        rc = lib.lz4flex_paged_read_ranges(None, p[0], P, *p[1:6], n, *p[6:9], m, *p[9:13], max_items, _ptr(scratch) if scratch_cap else None,
                                           scratch_cap, _ptr(work), _lib.MEM_DEVICE, C.c_void_p(stream.cuda_stream))
        assert rc == 0, _lib.last_error()
        stream.synchronize()
        after = [x.cpu().numpy().view(a.dtype) for x, a in zip(d[:6], tables)]
        assert (d[6].cpu().numpy().view(np.uint32) == sid).all() and (d[10].cpu().numpy().view(np.uint64) == out_off).all()
        assert (scratch[scratch_cap:].cpu().numpy() == 0x11).all(), "scratch written behind scratch_cap"
        out, out_len, status = d[9].cpu().numpy(), d[11].cpu().numpy().view(np.uint32), d[12].cpu().numpy()
    for name, a, b in zip(TABLES, before, after):
        assert (a == b).all(), "the call wrote into " + name
    assert (out_len[m:] == 0x5A5A5A5A).all() and (status[m:] == 0x5A5A5A5A).all(), "results written past m"
    may = np.zeros(out.size, bool)
    for r in range(m):
        assert int(out_len[r]) <= room[r] and (status[r] == 0 or out_len[r] == 0), (r, ranges[r], int(status[r]), int(out_len[r]))
        may[int(out_off[r]):int(out_off[r]) + (int(out_len[r]) if int(status[r]) in STRICT else room[r])] = True
    wrong = np.nonzero(~may & (out != FILL))[0]
    assert wrong.size == 0, "bytes outside the ranges' regions were written, first at %d" % int(wrong[0])
    return [int(v) for v in status[:m]], [int(v) for v in out_len[:m]], [out[int(o):int(o) + int(k)].tobytes() for o, k in zip(out_off, out_len)]


def expect_from_source(s, ranges, plan):
    """(status, out_len, bytes) for tables that tell the truth"""
    out = []
    for (i, off, length), rec, pre in zip(ranges, plan.recs, plan.pre):
        out.append((0, rec.len, s.data[i][off:off + rec.len]) if pre in (None, 0) else (pre, 0, b""))
    return out


def check(got, want, what):
    st, ln, by = got
    for r, (ws, wl, wb) in enumerate(want):
        assert (st[r], ln[r]) == (ws, wl), (what, r, (st[r], ln[r]), (ws, wl))
        if ws == 0:
            assert by[r] == wb, (what, r, "bytes")


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("name", SETS)
def test_ranges_are_the_sources_bytes(lib, name, mem):
    s = the_set(name)
    t = s.t
    ranges, count = ranges_of(t)
    if name.startswith("n37"):
        assert all(count[c] > 0 for c in CLASSES), count                      # no class drops out silently
    if name == "short@64":
        assert int(s.status[0]) == R.E_OUTPUT_TOO_SMALL and 0 < t.in_done[0] < len(s.data[0]) and t.n_pages[0] == 5
    plan = R.plan(t, ranges)
    assert R.E_OUTPUT_TOO_SMALL not in plan.pre and [p for p in plan.pre if p == R.E_INVALID_ARG] == [R.E_INVALID_ARG]
    got = run_read(lib, s.arrays, s.P, ranges, mem, plan.items_needed, plan.scratch_needed)
    check(got, expect_from_source(s, ranges, plan), (name, mem))


def test_every_class_is_covered_by_the_single_stream_sets():
    total = dict.fromkeys(CLASSES, 0)
    for name in SETS[3:]:
        for c, v in ranges_of(the_set(name).t)[1].items():
            total[c] += v
    assert all(total[c] > 0 for c in CLASSES), total


def test_host_and_device_agree_and_oversized_capacities_change_nothing(lib):
    s = the_set("n37@64")
    ranges, _ = ranges_of(s.t)
    plan = R.plan(s.t, ranges)
    host = run_read(lib, s.arrays, s.P, ranges, "host", 0, 0)
    exact = run_read(lib, s.arrays, s.P, ranges, "device", plan.items_needed, plan.scratch_needed)
    wide = run_read(lib, s.arrays, s.P, ranges, "device", 4 * plan.items_needed + 7, 2 * plan.scratch_needed + 64)
    bound = sum(R.pages_bound(length, s.P) for _, _, length in ranges if length != R.WHOLE) + sum(s.t.n_pages)
    assert plan.items_needed <= bound
    assert host == exact == wide


def test_capacities_one_short(lib):
    """max_items and scratch_cap one short of the need of the last range with a head: exactly the model's ranges report
    E_OUTPUT_TOO_SMALL, their regions are untouched (run_read checks it), all others are correct"""
    s = the_set("n37@509")
    t = s.t
    ranges, _ = ranges_of(t)
    full = R.plan(t, ranges)
    q = max(r for r, rec in enumerate(full.recs) if rec.head and full.pre[r] is None)
    items_short, scratch_short = full.slot[q] + full.recs[q].nb - 1, full.head_off[q] + full.recs[q].head_bytes - 1
    for max_items, scratch_cap in ((items_short, full.scratch_needed), (full.items_needed, scratch_short), (items_short, scratch_short), (0, 0)):
        plan = R.plan(t, ranges, max_items, scratch_cap)
        refused = [r for r, p in enumerate(plan.pre) if p == R.E_OUTPUT_TOO_SMALL]
        assert q in refused and (max_items or len(refused) == sum(1 for rec in full.recs if rec.nb))
        got = run_read(lib, s.arrays, s.P, ranges, "device", max_items, scratch_cap)
        check(got, expect_from_source(s, ranges, plan), ("short", max_items, scratch_cap))
        assert [r for r, st in enumerate(got[0]) if st == R.E_OUTPUT_TOO_SMALL] == refused


def partial_decoder(arrays, P, t, ranges):
    """decode_partial for the model's read(): every item of the ranges decoded by ONE lz4flex_decompress_batch_partial over those pages
    alone"""
    from lz4_flex_amd import block
    plan = R.plan(t, ranges)
    keys = sorted({(it.entry, it.in_len, it.target) for rec, pre in zip(plan.recs, plan.pre) if pre is None for it in R.items(t, rec)})
    if not keys:
        return lambda *k: (_ for _ in ()).throw(AssertionError("no item"))
    out_off = np.zeros(len(keys), np.uint64)
    out_off[1:] = np.cumsum([k[2] for k in keys[:-1]])
    out = np.zeros(sum(k[2] for k in keys) + 1, np.uint8)
    out_len, status = block.decompress_batch_partial(arrays["pages"], [k[0] * P for k in keys], [k[1] for k in keys], out, out_off, [k[2] for k in keys])
    table = {k: (int(st), out[int(o):int(o) + int(n)].tobytes()) for k, st, o, n in zip(keys, status, out_off, out_len)}
    return lambda entry, in_len, target: table[entry, in_len, target]


def sequences(block):
    """[(position of the token, position of the offset or None, output bytes behind its literals)] of an LZ4 block"""
    out, ip, op = [], 0, 0
    while ip < len(block):
        tok_at, tok = ip, block[ip]
        ip += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = block[ip]
                ip += 1
                lit += b
                if b != 255:
                    break
        ip += lit
        op += lit
        if ip >= len(block):
            out.append((tok_at, None, op))
            break
        out.append((tok_at, ip, op))
        ip += 2
        ml = (tok & 15) + 4
        if (tok & 15) == 15:
            while True:
                b = block[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        op += ml
    return out


@pytest.mark.parametrize("mem", ["host", "device"])
def test_damaged_pages(lib, mem):
    """an offset of 0 in the middle of one page, and another page whose page_len ends it early, behind a sequence's literals: ranges that
    want bytes in front of the damage are still correct, ranges that need bytes behind it report the partial decoder's code or
    E_EXPECTED_ANOTHER_BYTE, ranges elsewhere are unaffected"""
    s = the_set("n37@509")
    t, P = s.t, s.P
    i = max(range(t.n), key=lambda x: t.n_pages[x])
    first, k = t.page_off[i], t.n_pages[i]
    assert k >= 6
    arrays = {name: a.copy() for name, a in s.arrays.items()}
    hit = {}
    for kind, e in (("offset", first + 1), ("early", first + 3)):
        blk = bytes(arrays["pages"][e * P:e * P + t.page_len[e]])
        seqs = [q for q in sequences(blk) if q[1] is not None and q[2] >= 8]
        assert seqs, kind
        tok_at, off_at, clean = seqs[0]
        if kind == "offset":
            arrays["pages"][e * P + off_at:e * P + off_at + 2] = 0
        else:
            arrays["page_len"][e] = off_at                                    # the page ends behind that sequence's literals
        size = (t.page_src[e + 1] if e + 1 < first + k else t.in_done[i]) - t.page_src[e]
        assert clean < size
        hit[e] = (t.page_src[e], clean)
    ranges, _ = ranges_of(t)
    for e, (start, clean) in hit.items():
        ranges += [(i, start, clean), (i, start + 2, clean - 2), (i, start + 2, clean - 1), (i, start, clean + 1), (i, start - 5, clean + 5),
                   (i, start - 5, clean + 6), (i, start + clean, 4)]
    t2 = model_of(arrays, P)
    plan = R.plan(t2, ranges)
    want = R.read(t2, ranges, partial_decoder(arrays, P, t2, ranges))
    got = run_read(lib, arrays, P, ranges, mem, plan.items_needed, plan.scratch_needed)
    check(got, [(st, n, by) for st, n, by in want], ("damage", mem))
    in_front = behind = 0
    for r, ((j, off, length), rec, (st, n, by)) in enumerate(zip(ranges, plan.recs, want)):
        touched = {rec.first + rec.j0 + x for x in range(rec.nb)} & set(hit) if j == i and rec.len else set()
        needs = any(off + rec.len > hit[e][0] + hit[e][1] for e in touched)
        if j >= t.n:
            assert st == R.E_INVALID_ARG
        elif not needs:                                                       # elsewhere, or in front of the damage: the source's bytes
            assert st == 0 and got[2][r] == s.data[j][off:off + rec.len], (r, ranges[r])
            in_front += bool(touched)
        else:
            assert st not in STRICT and got[0][r] == st, (r, ranges[r], st)
            behind += 1
    codes = {st for st, _, _ in want}
    assert in_front >= 4 and behind >= 6 and R.E_EXPECTED_ANOTHER_BYTE in codes and len(codes - set(STRICT)) >= 2, (in_front, behind, codes)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("kind", ["reversed", "n_pages"])
def test_hostile_tables(lib, kind, mem):
    """page_src of one stream reversed / n_pages[i] = C_i + 5: wrong numbers, not wild pointers.  Affected ranges report E_INVALID_ARG or
    a decode error, the canaries are intact (run_read checks them), the other streams' ranges are correct"""
    s = the_set("n37@64")
    t, P = s.t, s.P
    i = max(range(t.n), key=lambda x: t.n_pages[x])
    first, k, C_i = t.page_off[i], t.n_pages[i], t.page_off[i + 1] - t.page_off[i]
    arrays = {name: a.copy() for name, a in s.arrays.items()}
    if kind == "reversed":
        arrays["page_src"][first:first + k] = arrays["page_src"][first:first + k][::-1].copy()
    else:
        arrays["n_pages"][i] = C_i + 5
    ranges, _ = ranges_of(t)
    t2 = model_of(arrays, P)
    plan = R.plan(t2, ranges)
    want = R.read(t2, ranges, partial_decoder(arrays, P, t2, ranges))
    got = run_read(lib, arrays, P, ranges, mem, plan.items_needed, plan.scratch_needed)
    check(got, want, (kind, mem))
    refused = 0
    for r, ((j, off, length), rec) in enumerate(zip(ranges, R.plan(t, ranges).recs)):
        if j != i and j < t.n:
            assert got[0][r] == 0 and got[2][r] == s.data[j][off:off + rec.len], (r, ranges[r])
        elif j == i and got[0][r] != 0:
            refused += 1
    assert refused >= 3 and R.E_INVALID_ARG in {got[0][r] for r, (j, _, _) in enumerate(ranges) if j == i}


def test_decompress_partial_setting_and_python_forms(lib):
    import torch
    from lz4_flex_amd import block
    s = the_set("n37@509")
    t = s.t
    ranges, _ = ranges_of(t)
    plan = R.plan(t, ranges)
    want = expect_from_source(s, ranges, plan)
    try:
        for v in (0, 1):
            assert lib.lz4flex_set_tuning(None, b"decompress_partial", v) == 0
            for mem in ("host", "device"):
                check(run_read(lib, s.arrays, s.P, ranges, mem, plan.items_needed + 5, plan.scratch_needed), want, ("decompress_partial", v, mem))
    finally:
        assert lib.lz4flex_set_tuning(None, b"decompress_partial", 1) == 0
    raw = run_read(lib, s.arrays, s.P, ranges, "device", plan.items_needed, plan.scratch_needed)
    sid, off, length = ([r[k] for r in ranges] for k in range(3))
    paged = block.PagedStreams(page_size=s.P, status=s.status, **s.arrays)
    got, st = block.read_paged_ranges(paged, sid, off, length)
    assert [int(v) for v in st] == raw[0] and got == raw[2]
    dev = block.PagedStreams(page_size=s.P, status=_dev(s.status), **{k: _dev(v) for k, v in s.arrays.items()})
    for lens in (length, torch.tensor(length, dtype=torch.int64, device="cuda")):      # host-visible lengths, and lengths on the device
        out, out_off, out_len, st = block.read_paged_ranges_device(dev, sid, off, lens)
        torch.cuda.synchronize()
        h = out.cpu().numpy()
        assert st.cpu().tolist() == raw[0] and out_len.cpu().tolist() == raw[1]
        assert [h[int(o):int(o) + int(n)].tobytes() for o, n in zip(out_off.cpu().tolist(), out_len.cpu().tolist())] == raw[2]
    # whole streams: length 0xFFFFFFFF with off 0
    n = t.n
    out, out_off, out_len, st = block.read_paged_ranges_device(dev, list(range(n)), [0] * n, [R.WHOLE] * n)
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert st.cpu().tolist() == [0] * n
    assert [h[int(o):int(o) + int(k)].tobytes() for o, k in zip(out_off.cpu().tolist(), out_len.cpu().tolist())] == s.data
