"""lz4_flex_amd/csrc/frame_range.h on the CPU: where a byte range of a frame's content lies in the block table, which ranges start
with a head, and how ranges are cut into passes.

The expected values never come from the header: a range is located with Python's `bisect` over the same table, the head rule and the
pass rule are restated here in their own words."""
import bisect
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sim", "frame_range_shim.cpp")
HDR = os.path.join(ROOT, "lz4_flex_amd", "csrc", "frame_range.h")
SO = os.path.join(ROOT, "tests", "sim", "libframe_range_shim.so")
STORED = 0x80000000
DEFAULT_PASS = 256 << 20

_m = None


def shim():
    global _m
    if _m is None:
        if not os.path.exists(SO) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(SO):
            subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-Wall", SRC, "-o", SO])
        m = C.CDLL(SO)
        u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
        for name in ("fr_rec_bytes", "fr_head_align", "fr_pass_slots_max"):
            getattr(m, name).restype = C.c_uint64
        m.fr_locate.restype = None
        m.fr_locate.argtypes = [u64p, u32p, C.c_uint32, C.c_uint64, C.c_uint64, u64p]
        m.fr_plan.restype = C.c_uint32
        m.fr_plan.argtypes = [u64p, u32p, C.c_uint32, u64p, u64p, C.c_uint32, u64p, C.c_uint64, u64p]
        _m = m
    return _m


def _p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


class Table:
    def __init__(self, sizes, stored):
        self.co = np.zeros(len(sizes) + 1, np.uint64)
        self.co[1:] = np.cumsum(np.array(sizes, np.uint64))
        self.lw = np.array([(17 + 3 * i) | (STORED if s else 0) for i, s in enumerate(stored)], np.uint32)
        self.off = [int(v) for v in self.co]
        self.stored = list(stored)
        self.S = self.off[-1]

    def locate(self, off, length):
        out = np.zeros(5, np.uint64)
        shim().fr_locate(_p64(self.co), _p32(self.lw), len(self.lw), off, length, _p64(out))
        return [int(v) for v in out]

    def expected(self, off, length):
        """[clipped length, b0, nb, head, head_bytes] by bisect: the block of a byte is the last one that starts at or before it"""
        n = min(length, self.S - off) if off < self.S else 0
        if n == 0:
            return [0, 0, 0, 0, 0]
        b0 = bisect.bisect_right(self.off, off) - 1
        b1 = bisect.bisect_right(self.off, off + n - 1) - 1
        assert self.off[b0] <= off < self.off[b0 + 1] and self.off[b1] <= off + n - 1 < self.off[b1 + 1]
        s = off - self.off[b0]
        head = 1 if s > 0 and not self.stored[b0] else 0
        head_bytes = min(off + n, self.off[b0 + 1]) - self.off[b0] if head else 0
        return [n, b0, b1 - b0 + 1, head, head_bytes]

    def plan(self, ranges, pass_bytes, cost=None):
        m = len(ranges)
        off = np.array([o for o, _ in ranges], np.uint64)
        ln = np.array([n for _, n in ranges], np.uint64)
        per = np.zeros(4 * max(m, 1), np.uint64)
        c = None if cost is None else np.array(cost, np.uint64)
        passes = shim().fr_plan(_p64(self.co), _p32(self.lw), len(self.lw), _p64(off), _p64(ln), m, None if c is None else _p64(c), pass_bytes,
                                _p64(per))
        return passes, per.reshape(-1, 4)[:m].astype(object)


def _random_table(rnd, n, big=False):
    sizes = [0 if rnd.random() < 0.1 else rnd.choice([1, 7, 100, 65536, rnd.randrange(1, 65537)]) for _ in range(n)]
    if big:
        sizes[rnd.randrange(n // 2)] = 5 << 30                    # (a table need not come from a real frame: content offsets above 4 GiB)
    if sum(sizes) == 0:
        sizes[0] = 5
    return Table(sizes, [rnd.random() < 0.4 for _ in range(n)])


def _edge_ranges(t, rnd):
    out = []
    for c in sorted(set(t.off)):
        for d in (-1, 0, 1):
            for n in (0, 1, 2, 17, 65536, 70000):
                if c + d >= 0:
                    out.append((c + d, n))
    for b in range(len(t.stored)):                                 # ends exactly on a block boundary, from inside and from a start
        if t.off[b + 1] > t.off[b]:
            out.append((t.off[b], t.off[b + 1] - t.off[b]))
            out.append((t.off[b] + (t.off[b + 1] - t.off[b]) // 2, t.off[b + 1] - t.off[b] - (t.off[b + 1] - t.off[b]) // 2))
    S = t.S
    out += [(S - 1, 5), (S, 5), (S + 10, 5), (S - 1, 0), (0, S), (0, S + 9), (0, 2 ** 64 - 1), (S - 1, 2 ** 64 - 1), (2 ** 64 - 1, 2 ** 64 - 1)]
    for _ in range(300):
        o = rnd.randrange(S + 3)
        out.append((o, rnd.choice([0, 1, rnd.randrange(1, 200000), S])))
    return out


def test_record_is_64_bytes():
    assert shim().fr_rec_bytes() == 64 and shim().fr_head_align() == 64


@pytest.mark.parametrize("seed,n,big", [(1, 1, False), (2, 2, False), (3, 40, False), (4, 300, False), (5, 300, True), (6, 9, True)])
def test_ranges_are_located_as_bisect_locates_them(seed, n, big):
    rnd = random.Random(seed)
    t = _random_table(rnd, n, big)
    if big:
        assert t.S > 1 << 32
    heads = 0
    for off, length in _edge_ranges(t, rnd):
        want = t.expected(off, length)
        assert t.locate(off, length) == want, (off, length)
        heads += want[3]
    assert heads > 0 or n < 40


def test_a_frame_without_blocks_or_content():
    t = Table([], [])
    assert t.locate(0, 5) == [0, 0, 0, 0, 0] and t.locate(7, 0) == [0, 0, 0, 0, 0]
    t = Table([0, 0], [True, False])
    assert t.locate(0, 5) == [0, 0, 0, 0, 0]


def _expected_passes(t, ranges, pass_bytes, cost=None):
    """a pass takes ranges while their costs add up to at most pass_bytes, and one at least; slots and head scratch count from the pass's start"""
    out, cur, bytes_, slot, heads = [], 0, 0, 0, 0
    first = True
    for i, (o, n) in enumerate(ranges):
        _, _, nb, head, hb = t.expected(o, n)
        c = (hb + 63) // 64 * 64 if cost is None else cost[i]
        if not first and bytes_ + c > pass_bytes:
            cur, bytes_, slot, heads = cur + 1, 0, 0, 0
        out.append([cur, slot, heads])
        slot += nb; heads += (hb + 63) // 64 * 64; bytes_ += c
        first = False
    totals = {}
    for (p, s, _), (o, n) in zip(out, ranges):
        totals[p] = max(totals.get(p, 0), s + t.expected(o, n)[2])
    return cur + 1 if ranges else 0, [row + [totals[row[0]]] for row in out]


@pytest.mark.parametrize("pass_bytes", [1, 64, 100000, DEFAULT_PASS])
def test_passes(pass_bytes):
    rnd = random.Random(11)
    t = _random_table(rnd, 200)
    ranges = [(rnd.randrange(t.S), rnd.choice([0, 1, 100, 70000, 300000])) for _ in range(500)]
    passes, per = t.plan(ranges, pass_bytes)
    want_passes, want = _expected_passes(t, ranges, pass_bytes)
    assert passes == want_passes and per.tolist() == want
    n_heads = sum(t.expected(o, n)[3] for o, n in ranges)
    assert n_heads > 100
    if pass_bytes == DEFAULT_PASS:
        assert passes == 1
    if pass_bytes == 1:
        # a head alone is over such a budget: the range behind a head starts a new pass, only head-less neighbours share one
        assert n_heads < passes < len(ranges)


def test_passes_by_a_callers_costs_and_one_range_per_pass():
    """MEM_HOST reads add their staged spans to the cost: with every cost above the pass size each range is a pass, slot 0, head_off 0"""
    rnd = random.Random(12)
    t = _random_table(rnd, 50)
    ranges = [(rnd.randrange(t.S), rnd.randrange(1, 100000)) for _ in range(64)]
    passes, per = t.plan(ranges, 1, cost=[2 + i for i in range(64)])
    assert passes == 64 and [list(r[:3]) for r in per] == [[i, 0, 0] for i in range(64)]
    cost = [rnd.randrange(0, 5000) for _ in range(64)]
    passes, per = t.plan(ranges, 9000, cost=cost)
    want_passes, want = _expected_passes(t, ranges, 9000, cost)
    assert passes == want_passes and per.tolist() == want and 10 < passes < 64
    huge = [2 ** 64 - 1] * 64                                       # (sums that would wrap: still one range per pass)
    assert t.plan(ranges, DEFAULT_PASS, cost=huge)[0] == 64
