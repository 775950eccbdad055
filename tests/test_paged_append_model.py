"""CPU tests of the rule of lz4flex_paged_append (include/lz4flex_amd.h): tests/paged_append_model.py over the oracle's exact encoder and
the fit rule (paged_model.by_encoder), on the streams of tests/paged_cases.py cut at several points -- every append equals ONE
paged_model.run over `tail ++ add` with the tail taken from the SOURCE, the pages decode to the concatenation, every page but a stream's
last holds at least Lfit(P) bytes and the pages bound holds after every step -- and lz4_flex_amd/csrc/paged_append.h (compiled for the
host with the system compiler, tests/sim/paged_append_shim.cpp) against the model's steps 1 to 4, on well-formed and on garbage tables.
No device, no compute calls."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import oracle_api as O
import paged_append_model as A
import paged_cases as K
import paged_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sim", "paged_append_shim.cpp")
HDRS = [os.path.join(ROOT, "lz4_flex_amd", "csrc", h) for h in ("paged_append.h", "paged_range.h")]
SO = os.path.join(ROOT, "tests", "sim", "libpaged_append_shim.so")
FIRST = 2                                   # page_off[0]: entries are absolute
CASES = [(64, 4096), (509, 20 * 1024)]      # (page size, the length text and JSON are cut to)
VARIANTS = ["fresh", "one", "inside", "last", "three"]


def oracle_round(windows):
    return [(O.compress(w), M.OK) for w in windows]


FIT = M.by_encoder(oracle_round)


def decode_partial(block, target):
    """the first `target` bytes of a page, by the oracle: the block is decoded whole (a page of these tests holds at most 64 KiB)"""
    kind, got = O.decompress(block, 1 << 17)
    return (A.OK, got[:target]) if kind == "ok" else (A.E_EXPECTED_ANOTHER_BYTE, b"")


def cuts_of(s, variant, P):
    """where stream s is cut: the first append takes s[:c0], the next s[c0:c1], ..."""
    n = len(s)
    inside = max(M.lfit_page(P) + 5, n // 2 + 3)                   # behind the first page, inside a later one ...
    inside = inside if inside < n else n // 2                      # ... or inside the only one
    c = {"fresh": [0], "one": [1], "inside": [inside], "last": [n - 1], "three": [n // 3, 2 * n // 3]}[variant]
    return [min(max(x, 0), n) for x in c] + [n]


def check_step(names, data, t, before, res, adds, P, wmin=0, wmax=0):
    """one append against the rule's own statement: the defining equality with the tail from the source, the pages against the oracle,
    the two invariants"""
    L = M.lfit_page(P)
    V, cap = [], []
    for i, s in enumerate(data):
        r = res.plan.recs[i]
        go = res.plan.pre[i] is A.GO and i in res.stage
        assert not go or res.stage[i] == s[r.base:r.S] + adds[i], names[i]
        V.append(s[r.base:r.S + len(adds[i])] if go else b"")
        cap.append(r.C - A.k0_of(r) if go else 0)
    want = M.run(V, P, cap, FIT, wmin, wmax)
    for i, (nm, s) in enumerate(zip(names, data)):
        r, k0 = res.plan.recs[i], A.k0_of(res.plan.recs[i])
        first = t.page_off[i]
        if not adds[i]:
            assert (res.status[i], res.stage_off[i], res.tail_src[i]) == (0, A.NO_STAGE, r.S), nm
            assert t.pages_of(i) == before.pages_of(i) and (t.n_pages[i], t.in_done[i]) == (before.n_pages[i], before.in_done[i]), nm
            continue
        assert res.tail_src[i] == r.base and res.stage_off[i] != A.NO_STAGE, nm
        assert (t.n_pages[i] - k0, t.in_done[i] - r.base, res.status[i]) == (want.n_pages[i], want.in_done[i], want.status[i]), nm
        assert [(pos - r.base, b) for pos, b in t.pages_of(i)[k0:]] == want.pages[i], nm
        assert t.pages_of(i)[:k0] == before.pages_of(i)[:k0], nm                 # entries in front of the reopened one are untouched
        # the pages decode to the concatenation
        S = t.in_done[i]
        pages = t.pages_of(i)
        ends = [pos for pos, _ in pages[1:]] + [S]
        at = 0
        for j, ((pos, block), end) in enumerate(zip(pages, ends)):
            assert pos == at and end > pos and len(block) <= P, (nm, j)
            assert O.decompress(block, end - pos) == ("ok", s[pos:end]), (nm, j)
            assert j + 1 == len(pages) or end - pos >= L, (nm, j, end - pos)      # every page but the last: at least Lfit(P) bytes
            at = end
        assert at == S and t.n_pages[i] <= M.pages_bound(S, P), nm
    return want


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("P,cut", CASES, ids=["P%d" % p for p, _ in CASES])
def test_appends_equal_one_paged_run_over_tail_and_add(P, cut, variant):
    cases = K.streams(P, cut=cut, zeros=16 * 1024)
    names, data = [nm for nm, _ in cases], [s for _, s in cases]
    t = A.empty_tables(P, [M.pages_bound(len(s), P) for s in data], first=FIRST)      # the bound for the final length always suffices
    cuts = [cuts_of(s, variant, P) for s in data]
    done = [0] * len(data)
    reopened = 0
    for step in range(max(len(c) for c in cuts)):
        adds = [s[done[i]:c[step]] if step < len(c) else b"" for i, (s, c) in enumerate(zip(data, cuts))]
        before = t.copy()
        res = A.run(t, adds, FIT, decode_partial)
        assert res.status == [0] * len(data), (step, res.status)
        check_step(names, data, t, before, res, adds, P)
        reopened += sum(1 for i, r in enumerate(res.plan.recs) if adds[i] and r.k)
        done = [done[i] + len(a) for i, a in enumerate(adds)]
        assert t.in_done == done
    assert done == [len(s) for s in data]
    assert reopened >= (0 if variant == "fresh" else 8)
    longest_add = max(len(s) for s in data)
    assert res.rounds is None or res.rounds.rounds <= M.rounds_bound(M.windows_of(P)[1] + longest_add, P)


@pytest.mark.parametrize("P", [P for P, _ in CASES])
def test_a_tail_page_that_holds_a_whole_window(P):
    """a run of zeros at window_max = 4 P: every page holds window_max bytes, so the reopened tail is exactly a window long -- the
    longest a table of lz4flex_compress_paged can name -- and one byte more in in_done is a contradiction"""
    wmin, wmax = P, 4 * P
    assert len(O.compress(bytes(wmax))) <= P
    s = bytes(8 * wmax)
    t = A.empty_tables(P, [M.pages_bound(len(s), P)], first=FIRST)
    res = A.run(t, [s[:3 * wmax]], FIT, decode_partial, wmin, wmax)
    assert res.status == [0] and t.n_pages == [3] and [pos for pos, _ in t.pages_of(0)] == [0, wmax, 2 * wmax]
    before = t.copy()
    res = A.run(t, [s[3 * wmax:]], FIT, decode_partial, wmin, wmax)
    assert res.plan.recs[0].T == wmax and res.tail_src == [2 * wmax] and res.status == [0]
    check_step(["zeros"], [s], t, before, res, [s[3 * wmax:]], P, wmin, wmax)
    assert t.n_pages == [8] and t.in_done == [len(s)]
    worse = before.copy()
    worse.in_done[0] += 1
    assert A.plan(worse, [5], wmax).pre == [A.E_INVALID_ARG] and A.plan(before, [5], wmax).pre == [A.GO]


def test_a_stream_out_of_pages_leaves_a_valid_prefix():
    P = 64
    cases = K.streams(P, cut=2048, zeros=4096)
    names, data = [nm for nm, _ in cases], [s for _, s in cases]
    half = [len(s) // 2 for s in data]
    t = A.empty_tables(P, [M.pages_bound(h, P) for h in half], first=FIRST)
    assert A.run(t, [s[:h] for s, h in zip(data, half)], FIT, decode_partial).status == [0] * len(data)
    # no room behind n_pages: C == k for every stream that filled its bound, and at most a page more for the others
    before = t.copy()
    adds = [s[h:] for s, h in zip(data, half)]
    res = A.run(t, adds, FIT, decode_partial)
    short = [i for i, st in enumerate(res.status) if st == A.E_OUTPUT_TOO_SMALL]
    assert short and set(res.status) <= {0, A.E_OUTPUT_TOO_SMALL}
    for i, (nm, s) in enumerate(zip(names, data)):
        base = res.tail_src[i]
        assert (base <= t.in_done[i] <= len(s)) if adds[i] else t.in_done[i] == half[i], nm
        assert (t.in_done[i] == len(s)) == (res.status[i] == 0), nm
        got = b"".join(O.decompress(b, 1 << 17)[1] for _, b in t.pages_of(i))
        assert got == s[:t.in_done[i]], nm                                       # a valid prefix [0, in_done)
        if i in short:
            assert t.n_pages[i] == t.page_off[i + 1] - t.page_off[i], nm
            assert res.stage[i][t.in_done[i] - base:] == s[t.in_done[i]:], nm     # the bytes not yet paged are in the stage
    # no rounds at all: the reopened page leaves the table, nothing is lost
    t2 = before.copy()
    res = A.run(t2, adds, FIT, decode_partial, max_rounds=0)
    for i in range(len(data)):
        if adds[i]:
            k0 = A.k0_of(res.plan.recs[i])
            assert (res.status[i], t2.n_pages[i], t2.in_done[i]) == (A.E_OUTPUT_TOO_SMALL, k0, res.tail_src[i]), names[i]
            assert res.stage[i] == data[i][res.tail_src[i]:]


# ---- paged_append.h, compiled for the host ----------------------------------------------------------------------------------------------
_m = None


def shim():
    global _m
    if _m is None:
        if not os.path.exists(SO) or max(os.path.getmtime(p) for p in [SRC] + HDRS) > os.path.getmtime(SO):
            subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-Wall", SRC, "-o", SO])
        m = C.CDLL(SO)
        u64p, u32p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
        m.pa_rec_bytes.restype = m.pa_stage_bound.restype = m.pa_plan.restype = C.c_uint64
        m.pa_stage_bound.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
        m.pa_plan.argtypes = [u64p, u32p, u32p, u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, u32p, C.c_uint64, i32p, u64p]
        _m = m
    return _m


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def shim_plan(t, add_len, window_max, stage_cap):
    """(pre with -1 for GO, rows of [base, T, need, slot, stage_off, tail_src, k0, room], total)"""
    n = t.n
    page_off = np.array(t.page_off, np.uint64)
    cols = [np.array(list(a) + [0], np.uint32) for a in (t.page_len, t.page_src, t.n_pages, t.in_done, add_len)]
    pre, out = np.zeros(n + 1, np.int32), np.zeros(8 * (n + 1), np.uint64)
    total = shim().pa_plan(_p(page_off, C.c_uint64), *[_p(a, C.c_uint32) for a in cols[:4]], n, t.page_size, window_max, _p(cols[4], C.c_uint32),
                           A.NO_STAGE if stage_cap is None else stage_cap, _p(pre, C.c_int32), _p(out, C.c_uint64))
    return [int(v) for v in pre[:n]], [[int(v) for v in out[8 * i:8 * i + 8]] for i in range(n)], int(total)


def model_plan(t, add_len, window_max, stage_cap):
    p = A.plan(t, add_len, window_max, stage_cap)
    rows = [[r.base, r.T, A.slot_bytes(r), p.slot[i], p.stage_off[i], p.tail_src[i], A.k0_of(r), r.C - A.k0_of(r) if p.pre[i] is A.GO else 0]
            for i, r in enumerate(p.recs)]
    return [-1 if v is A.GO else v for v in p.pre], rows, p.slot[-1]


def test_the_header_equals_the_model_on_well_formed_tables():
    assert shim().pa_rec_bytes() == 40
    for P, cut in CASES:
        cases = K.streams(P, cut=cut // 4, zeros=4096)
        data = [s for _, s in cases]
        wmax = M.windows_of(P)[1]
        t = A.empty_tables(P, [M.pages_bound(len(s), P) + 1 for s in data], first=FIRST)
        rng = random.Random(P)
        for step in range(3):
            add_len = [rng.choice([0, 1, 7, 300, 70000]) for _ in data]
            total = model_plan(t, add_len, wmax, None)[2]
            for cap in (None, 0, total - 1, total, total // 2):
                assert shim_plan(t, add_len, wmax, cap) == model_plan(t, add_len, wmax, cap), (P, step, cap)
            served = model_plan(t, add_len, wmax, total // 2)[0]
            assert (-1 in served and A.E_OUTPUT_TOO_SMALL in served) or total < 128
            assert total <= A.stage_bound(sum(add_len), len(data), wmax) == shim().pa_stage_bound(sum(add_len), len(data), wmax)
            third = [s[len(s) * step // 3:len(s) * (step + 1) // 3] for s in data]
            assert A.run(t, third, FIT, decode_partial).status == [0] * len(data)
        # each contradiction of step 2, one stream at a time, on the tables as they are now
        i = max(range(len(data)), key=lambda j: t.n_pages[j])
        e = t.page_off[i] + t.n_pages[i] - 1
        assert t.n_pages[i] >= 2

        def bad(**change):
            u = t.copy()
            for name, (at, v) in change.items():
                getattr(u, name)[at] = v
            add = [5] * len(data)
            got, want = shim_plan(u, add, wmax, None), model_plan(u, add, wmax, None)
            assert got == want
            return got[0]

        ok = bad()
        assert ok[i] == -1
        for change in (dict(page_len=(e, 0)), dict(page_len=(e, P + 1)), dict(page_src=(e, t.in_done[i])), dict(page_src=(e, t.in_done[i] + 9)),
                       dict(n_pages=(i, t.page_off[i + 1] - t.page_off[i] + 1)), dict(n_pages=(i, 0)), dict(in_done=(i, 0xFFFFFFFF - 4)),
                       dict(in_done=(i, t.page_src[e] + wmax + 1))):
            pre = bad(**change)
            assert pre[i] == A.E_INVALID_ARG and pre[:i] + pre[i + 1:] == ok[:i] + ok[i + 1:], change
        assert bad(in_done=(i, t.page_src[e] + wmax))[i] == -1 and bad(page_len=(e, P))[i] == -1
        down = t.copy()
        down.page_off[i + 1] = down.page_off[i] - 1                              # page_off counting down: stream i, and the count of i + 1
        assert shim_plan(down, [5] * len(data), wmax, None) == model_plan(down, [5] * len(data), wmax, None)
        assert model_plan(down, [5] * len(data), wmax, None)[0][i] == A.E_INVALID_ARG


def garbage(rng, rnd):
    n, P = rng.randrange(1, 7), rng.randrange(64, 264)
    wmax = P + rng.randrange(3000)
    page_off = [rng.randrange(3)]
    for _ in range(n):
        page_off.append(page_off[-1] - 1 if rnd % 7 == 6 and page_off[-1] and rng.randrange(4) == 0 else page_off[-1] + rng.randrange(9))
    entries = max(page_off)
    scale = 4000 if rnd % 2 else 0xFFFFFFFF
    page_len = [rng.randrange(P + 2 if rnd % 3 else scale) for _ in range(entries)]
    page_src = [rng.randrange(scale) for _ in range(entries)]
    n_pages, in_done = [rng.randrange(10) for _ in range(n)], [rng.randrange(scale) for _ in range(n)]
    if rnd % 4 == 0:                                   # mostly sound, so that streams go on
        for i in range(n):
            room = max(page_off[i + 1] - page_off[i], 0)
            n_pages[i] = rng.randrange(room + 1)
            if n_pages[i] == 0:
                in_done[i] = 0
                continue
            e = page_off[i] + n_pages[i] - 1
            page_len[e], page_src[e] = 1 + rng.randrange(P), rng.randrange(5000)
            in_done[i] = page_src[e] + 1 + rng.randrange(wmax)
    add_len = [0 if rng.randrange(4) == 0 else rng.randrange(1 << 32) if rng.randrange(5) == 0 else rng.randrange(3000) for _ in range(n)]
    stage_cap = None if rng.randrange(3) == 0 else rng.randrange(9000)
    return A.Tables(P, page_off, page_len, page_src, n_pages, in_done), add_len, wmax, stage_cap


def test_garbage_tables_never_give_a_stream_more_than_its_own():
    """2 000 seeded tables of random numbers: the header equals the model, and a stream that goes on reads one entry and one page of its
    own span, gets a slot inside stage_cap that holds its tail and its new bytes, and resumes inside its capacity"""
    rng = random.Random(20261)
    going = refused = contradicting = 0
    for rnd in range(2000):
        t, add_len, wmax, stage_cap = garbage(rng, rnd)
        got, want = shim_plan(t, add_len, wmax, stage_cap), model_plan(t, add_len, wmax, stage_cap)
        assert got == want, rnd
        pre, rows, total = got
        for i, (st, (base, T, need, slot, stage_off, tail_src, k0, room)) in enumerate(zip(pre, rows)):
            if st != -1:
                assert stage_off == A.NO_STAGE and room == 0 and (st != 0 or add_len[i] == 0), (rnd, i)
                refused += st == A.E_OUTPUT_TOO_SMALL
                contradicting += st == A.E_INVALID_ARG
                continue
            going += 1
            first, C, k = t.page_off[i], t.page_off[i + 1] - t.page_off[i], t.n_pages[i]
            assert C >= 0 and k <= C and k0 == max(k - 1, 0) and k0 + room == C, (rnd, i)
            assert need % 64 == 0 and need >= T + add_len[i] and T <= wmax, (rnd, i)
            assert stage_cap is None or stage_off + need <= stage_cap, (rnd, i)
            assert base + T + add_len[i] <= 0xFFFFFFFF, (rnd, i)
            if k:
                e = first + k - 1
                assert first <= e < first + C and 1 <= t.page_len[e] <= t.page_size and (base, T) == (t.page_src[e], t.in_done[i] - base), (rnd, i)
                assert T >= 1
            else:
                assert (base, T, t.in_done[i]) == (0, 0, 0), (rnd, i)
    assert going > 300 and refused > 30 and contradicting > 300


def test_the_stand_alone_driver_runs_clean_under_the_sanitizers(tmp_path):
    """tests/sim/paged_append_shim.cpp with its own main (the same garbage walk, checked in C++, every table exactly as long as the
    entries the streams own), built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a process of its own; nothing
    sanitized is loaded into Python"""
    exe = str(tmp_path / "paged_append_main")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DPAGED_APPEND_SHIM_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe]
    if subprocess.call(cmd, stderr=subprocess.DEVNULL) != 0:
        pytest.skip("this compiler has no sanitizer runtimes")
    out = subprocess.check_output([exe]).decode()
    assert "all inside their bounds" in out, out
