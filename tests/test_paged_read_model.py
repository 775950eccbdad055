"""CPU tests of the rule of lz4flex_paged_read_ranges (include/lz4flex_amd.h): tests/paged_read_model.py and
lz4_flex_amd/csrc/paged_range.h (compiled for the host with the system compiler, tests/sim/paged_range_shim.cpp) over paged streams
built on the CPU -- tests/paged_model.py over the oracle's exact encoder and the fit rule, the construction tests/test_paged_model.py
uses.  The expected page of a byte never comes from either: it is a brute-force byte-to-page map; the expected bytes are the source's.
No device, no compute calls."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import oracle_api as O
import paged_cases as K
import paged_model as M
import paged_read_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sim", "paged_range_shim.cpp")
HDR = os.path.join(ROOT, "lz4_flex_amd", "csrc", "paged_range.h")
SO = os.path.join(ROOT, "tests", "sim", "libpaged_range_shim.so")
FIRST = 2                                   # page_off[0]: entries are absolute
CASES = [(64, 4096), (509, 20 * 1024)]      # (page size, the length text and JSON are cut to)

_m = None


def shim():
    global _m
    if _m is None:
        if not os.path.exists(SO) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(SO):
            subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-Wall", SRC, "-o", SO])
        m = C.CDLL(SO)
        u64p, u32p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
        m.pr_rec_bytes.restype = C.c_uint64
        m.pr_pages_bound.restype = m.pr_lfit_page.restype = C.c_uint32
        m.pr_pages_bound.argtypes = [C.c_uint32, C.c_uint32]
        m.pr_lfit_page.argtypes = [C.c_uint32]
        tables = [u64p, u32p, u32p, u32p, u32p, C.c_uint32, C.c_uint32]
        m.pr_locate.restype = None
        m.pr_locate.argtypes = tables + [C.c_uint32, C.c_uint32, C.c_uint32, u64p]
        m.pr_plan.restype = C.c_uint64
        m.pr_plan.argtypes = tables + [u32p, u32p, u32p, C.c_uint32, C.c_uint64, C.c_uint64, i32p, u64p, u64p, C.c_uint64]
        _m = m
    return _m


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class CTables:
    """a paged_read_model.Tables as the arrays the header takes (an empty array still has an address)"""

    def __init__(self, t):
        self.t = t
        self.page_off = np.array(t.page_off, np.uint64)
        self.cols = [np.array(list(a) + [0], np.uint32) for a in (t.page_len, t.page_src, t.n_pages, t.in_done)]

    def args(self):
        return [_p(self.page_off, C.c_uint64)] + [_p(a, C.c_uint32) for a in self.cols] + [self.t.n, self.t.page_size]

    def locate(self, i, off, length):
        out = np.zeros(8, np.uint64)
        shim().pr_locate(*self.args(), i, off, length, _p(out, C.c_uint64))
        return [int(v) for v in out]

    def plan(self, ranges, max_items, scratch_cap, item_cap=1 << 16):
        m = len(ranges)
        sid, off, length = (np.array([r[k] for r in ranges] + [0], np.uint32) for k in range(3))
        pre, sums, items = np.zeros(m + 1, np.int32), np.zeros(2 * (m + 1), np.uint64), np.zeros(8 * item_cap, np.uint64)
        q = shim().pr_plan(*self.args(), _p(sid, C.c_uint32), _p(off, C.c_uint32), _p(length, C.c_uint32), m, max_items, scratch_cap,
                           _p(pre, C.c_int32), _p(sums, C.c_uint64), _p(items, C.c_uint64), item_cap)
        assert q <= item_cap
        return [int(v) for v in pre[:m]], [int(v) for v in sums], [[int(v) for v in items[8 * k:8 * k + 8]] for k in range(q)]


def model_items(t, p):
    """the model's plan in the shim's item layout"""
    out = []
    for r, (rec, pre) in enumerate(zip(p.recs, p.pre)):
        if pre is None:
            for it in R.items(t, rec):
                out.append([r, it.entry * t.page_size, it.in_len, it.target, int(it.head), p.head_off[r] if it.head else it.dst, it.copy_at, it.copy_len])
    return out


def oracle_round(windows):
    return [(O.compress(w), M.OK) for w in windows]


@pytest.fixture(scope="module")
def runs():
    """{P: (names, streams, Tables, {entry: block}, CTables)}: capacities of exactly the pages bound, entries from FIRST on; computed once"""
    out = {}
    for P, cut in CASES:
        cases = K.streams(P, cut=cut)
        data = [s for _, s in cases]
        cap = [M.pages_bound(len(s), P) for s in data]
        paged = M.run(data, P, cap, M.by_encoder(oracle_round))
        assert paged.status == [M.OK] * len(data)
        t, blocks = R.tables_of(paged, P, cap, first=FIRST)
        out[P] = ([nm for nm, _ in cases], data, t, blocks, CTables(t))
    return out


def page_map(t, i):
    """brute force: the page of every byte of stream i, and every page's [start, end)"""
    first, k, S = t.page_off[i], t.n_pages[i], t.in_done[i]
    starts = t.page_src[first:first + k] + [S]
    owner = []
    for j in range(k):
        owner += [j] * (starts[j + 1] - starts[j])
    assert len(owner) == S
    return owner, starts


def grid(starts, S):
    """(off, len): every page boundary -1 / 0 / +1, lengths 0, 1, 2, the page's size -1 / 0 / +1, three pages, to the end, past the
    end, whole; and offsets at and behind S"""
    offs = sorted({max(b + d, 0) for b in starts for d in (-1, 0, 1)} | {0, S, S + 1, S + 1000})
    out = []
    for off in offs:
        lens = {0, 1, 2, max(S - off, 0), max(S - off, 0) + 5, R.WHOLE}
        j = max([x for x in range(len(starts) - 1) if starts[x] <= off], default=None) if off < S else None
        if j is not None:
            size = starts[j + 1] - starts[j]
            three = starts[min(j + 3, len(starts) - 1)] - starts[j]
            lens |= {max(size - 1, 0), size, size + 1, three}
        out += [(off, n) for n in sorted(lens)]
    return out


@pytest.mark.parametrize("P", [P for P, _ in CASES])
def test_locate_equals_the_byte_to_page_map_and_the_header_equals_the_model(runs, P):
    names, data, t, blocks, ct = runs[P]
    checked = heads = 0
    for i, (nm, s) in enumerate(zip(names, data)):
        owner, starts = page_map(t, i)
        S = len(s)
        for off, length in grid(starts, S):
            rec = R.locate(t, i, off, length)
            n = min(length, S - off) if off < S else 0
            assert rec.len == n and not rec.no_stream, (nm, off, length)
            if n == 0:
                want = [0, 0, 0, 0, 0]
            else:
                j0, j1 = owner[off], owner[off + n - 1]
                head = off > starts[j0]
                want = [n, j0, j1 - j0 + 1, int(head), min(off + n, starts[j0 + 1]) - starts[j0] if head else 0]
                heads += head
            assert [rec.len, rec.j0, rec.nb, int(rec.head), rec.head_bytes] == want, (nm, off, length)
            assert R.sound(t, rec) and R.pages_bound(n, P) >= rec.nb and R.pages_bound(length, P) >= rec.nb, (nm, off, length)
            assert ct.locate(i, off, length) == want + [0, 0, t.n_pages[i]], (nm, off, length)
            # the items tile the range's region: the head's copy from 0, every body where the one in front of it ends
            at = 0
            for it in R.items(t, rec):
                assert (0 if it.head else it.dst) == at and it.in_len == len(blocks[it.entry]) <= P, (nm, off, length)
                at += it.copy_len if it.head else it.target
                assert not it.head or (it.target == rec.head_bytes and it.copy_at + it.copy_len == it.target)
            assert at == n, (nm, off, length)
            checked += 1
    assert checked > 500 and heads > 100
    assert R.locate(t, t.n, 0, 5).no_stream and ct.locate(t.n, 0, 5) == [0, 0, 0, 0, 0, 0, 1, 0]
    assert shim().pr_rec_bytes() == 48


@pytest.mark.parametrize("P", [P for P, _ in CASES])
def test_the_pages_bound_is_attained_on_the_incompressible_stream(runs, P):
    names, data, t, blocks, ct = runs[P]
    i = names.index("noise")
    L = M.lfit_page(P)
    first, k = t.page_off[i], t.n_pages[i]
    src = t.page_src[first:first + k]
    assert src == [j * L for j in range(k)] and k >= 3
    for span in range(2, k + 1):                       # from the last byte of page j to the first byte of the page span - 1 later
        for j in range(k - span + 1):
            off, last = src[j] + L - 1, src[j + span - 1]
            n = last - off + 1
            rec = R.locate(t, i, off, n)
            assert rec.nb == span == R.pages_bound(n, P) == shim().pr_pages_bound(n, P), (span, j)
            assert R.pages_bound(n - 1, P) >= R.locate(t, i, off, n - 1).nb == span - 1
    for length in (0, 1, 2, L + 1, L + 2, 2 * L + 2, 0xFFFFFFFF):
        assert R.pages_bound(length, P) == shim().pr_pages_bound(length, P) == (length if length < 2 else 2 + (length - 2) // L)
    assert R.pages_bound(100, 63) == 0 == shim().pr_pages_bound(100, 63) and shim().pr_pages_bound(100, (4 << 20) + 1) == 0
    assert shim().pr_lfit_page(P) == L


def some_ranges(t, names, rng):
    """ranges over every stream, in a shuffled order: heads, whole pages, whole streams, empty ones, a stream that does not exist"""
    out = []
    for i in range(t.n):
        S, first, k = t.in_done[i], t.page_off[i], t.n_pages[i]
        out += [(i, 0, R.WHOLE), (i, S, 4), (i, 0, 0)]
        for _ in range(6):
            off = rng.randrange(S + 1)
            out.append((i, off, rng.choice([1, 7, 64, 300, 2000, R.WHOLE])))
        for j in range(min(k, 3)):
            out.append((i, t.page_src[first + j], 50))
    out.append((t.n, 0, 10))
    rng.shuffle(out)
    return out + [(i, 0, R.WHOLE) for i in range(t.n - 3, t.n)]          # behind the last head: ranges from their pages' first bytes


@pytest.mark.parametrize("P", [P for P, _ in CASES])
def test_the_capacities_refuse_exactly_the_ranges_the_rule_names(runs, P):
    names, data, t, blocks, ct = runs[P]
    ranges = some_ranges(t, names, random.Random(P))
    full = R.plan(t, ranges)
    assert full.pre.count(None) > 30 and R.E_OUTPUT_TOO_SMALL not in full.pre
    q = max(r for r, rec in enumerate(full.recs) if rec.head and full.pre[r] is None)          # the last range with a head
    assert any(rec.nb for rec in full.recs[q + 1:])
    items_short = full.slot[q] + full.recs[q].nb - 1
    scratch_short = full.head_off[q] + full.recs[q].head_bytes - 1
    # restated: a range with bytes is refused iff the pages of the ranges up to and including it outnumber max_items ...
    total, by_items = 0, set()
    for r, rec in enumerate(full.recs):
        total += rec.nb
        if rec.len and total > items_short:
            by_items.add(r)
    assert q in by_items and len(by_items) > 1
    for max_items, scratch_cap, want in ((items_short, None, by_items), (None, scratch_short, {q}), (items_short, scratch_short, by_items),
                                         (full.items_needed, full.scratch_needed, set()), (0, 0, {r for r, rec in enumerate(full.recs) if rec.nb})):
        p = R.plan(t, ranges, max_items, scratch_cap)
        assert {r for r, st in enumerate(p.pre) if st == R.E_OUTPUT_TOO_SMALL} == want, (max_items, scratch_cap)
        assert [st for r, st in enumerate(p.pre) if r not in want] == [st for r, st in enumerate(full.pre) if r not in want]
        big = 1 << 62
        pre, sums, items = ct.plan(ranges, big if max_items is None else max_items, big if scratch_cap is None else scratch_cap)
        assert pre == [-1 if st is None else st for st in p.pre], (max_items, scratch_cap)
        assert sums == [v for pair in zip(p.slot, p.head_off) for v in pair]
        assert items == model_items(t, p)
    # ... and the whole rule gives the source's bytes for every range that is served
    def decode_partial(entry, in_len, target):
        i = max(x for x in range(t.n) if t.page_off[x] <= entry)
        j = entry - t.page_off[i]
        end = t.page_src[entry + 1] if j + 1 < t.n_pages[i] else t.in_done[i]
        kind, got = O.decompress(blocks[entry][:in_len], end - t.page_src[entry])
        assert kind == "ok"
        return R.OK, got[:target]

    for (i, off, length), (st, out_len, got), pre in zip(ranges, R.read(t, ranges, decode_partial, items_short, scratch_short), full.pre):
        if st == R.OK:
            assert got == data[i][off:off + out_len] and out_len == (min(length, len(data[i]) - off) if off < len(data[i]) else 0)
        else:
            assert (out_len, got) == (0, None) and st == (R.E_OUTPUT_TOO_SMALL if pre is None else pre)


def test_garbage_tables_never_give_an_item_outside_its_bounds():
    """1 000 seeded tables of random numbers: the header equals the model, and no item reads outside its stream's entries or writes
    outside its range's [0, out_len) or its head slot"""
    rng = random.Random(20251)
    planned = n_items = 0
    for rnd in range(1000):
        n, P = rng.randrange(1, 6), rng.randrange(64, 264)
        page_off = [rng.randrange(3)]
        for _ in range(n):
            page_off.append(page_off[-1] + rng.randrange(9))
        entries = page_off[-1]
        scale = 1000 if rnd % 2 else 0xFFFFFFFF
        page_len = [rng.randrange(P + 2 if rnd % 3 else scale) for _ in range(entries)]
        page_src = [rng.randrange(scale) for _ in range(entries)]
        tame = rnd % 4 == 0                            # mostly ascending, so that ranges get planned
        if tame:
            for i in range(n):
                at = 0
                for e in range(page_off[i], page_off[i + 1]):
                    page_src[e] = at
                    at += 1 + rng.randrange(300)
        t = R.Tables(P, page_off, page_len, page_src, [rng.randrange(12) for _ in range(n)], [rng.randrange(2000 if tame else scale) for _ in range(n)])
        ranges = [(rng.randrange(n + 1), rng.randrange(2100 if tame else scale), R.WHOLE if rng.randrange(5) == 0 else rng.randrange(900)) for _ in range(40)]
        max_items, scratch_cap = rng.randrange(60), rng.randrange(4000)
        p = R.plan(t, ranges, max_items, scratch_cap)
        pre, sums, items = CTables(t).plan(ranges, max_items, scratch_cap)
        assert pre == [-1 if st is None else st for st in p.pre], rnd
        assert items == model_items(t, p), rnd
        assert len(items) <= max_items
        for r, in_off, in_len, target, head, out_off, copy_at, copy_len in items:
            i, rec = ranges[r][0], p.recs[r]
            e = in_off // P
            assert in_off % P == 0 and page_off[i] <= e < page_off[i + 1] and in_len <= P and target >= 1, (rnd, r)
            if head:
                assert out_off == p.head_off[r] and target <= rec.head_bytes and out_off + target <= scratch_cap, (rnd, r)
                assert copy_at + copy_len <= target and copy_len <= rec.len, (rnd, r)
            else:
                assert out_off + target <= rec.len, (rnd, r)
        planned += p.pre.count(None)
        n_items += len(items)
    assert planned > 500 and n_items > 500


def test_the_stand_alone_driver_runs_clean_under_the_sanitizers(tmp_path):
    """tests/sim/paged_range_shim.cpp with its own main (the same garbage walk, checked in C++), built with AddressSanitizer and
    UndefinedBehaviorSanitizer where the compiler has their runtimes, plainly where it has not"""
    exe = str(tmp_path / "paged_range_main")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DPAGED_RANGE_SHIM_MAIN", SRC, "-o", exe]
    if subprocess.call(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base)
    out = subprocess.check_output([exe]).decode()
    assert "all inside their bounds" in out, out
