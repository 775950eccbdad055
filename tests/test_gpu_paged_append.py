"""GPU tests of lz4flex_paged_append (lz4_paged_append.hip): an append equals, byte for byte and entry for entry, ONE
lz4flex_compress_paged call over `tail ++ add` -- the tails taken from the source the test holds, dead streams empty -- for batches of 1
and of 37 streams, MEM_HOST and MEM_DEVICE, "compress_mode" 0, 1 and 2, fresh streams, streams that get nothing, one byte and several
pages' worth in one batch, with page_off[0] != 0.  Canaries stand around the page file, the tables, the results and the stage; entries in
front of the reopened one and at or behind the new n_pages stay as they were.  After three appends the read side returns the source.
Capacities, hostile tables and damaged tail pages leave their streams untouched and their neighbours correct."""
import ctypes as C

import numpy as np
import pytest

import paged_model as M
import test_gpu_paged as G

pytestmark = pytest.mark.gpu

GUARD, FILL, CANARY, EXTRA, FIRST_ENTRY = G.GUARD, G.FILL, G.CANARY, G.EXTRA, G.FIRST_ENTRY
CANARY64 = 0x5A5A5A5A5A5A5A5A
NO_STAGE = 0xFFFFFFFFFFFFFFFF
E_OUTPUT_TOO_SMALL, E_EXPECTED_ANOTHER_BYTE, E_INVALID_ARG = 1, 3, 64
MODES = G.MODES
BATCHES = [(64, "n37"), (509, "n37"), (4096, "n37"), (64, "n1:json")]


@pytest.fixture(scope="module")
def lib():
    from lz4_flex_amd import _lib
    lib = _lib.load()
    if lib.lz4flex_device_count() < 1:
        pytest.fail("GPU tests need a device: " + _lib.last_error())
    return lib


@pytest.fixture
def settings(lib):
    from lz4_flex_amd import block

    def choose(mode, depth=None):
        block.set_compress_mode(mode)
        if depth:
            block.set_compress_depth(depth)
    yield choose
    block.set_compress_mode("fast")
    block.set_compress_depth(16)


class Tab:
    """paged streams between canaries: the page file with guard bytes around it, the tables and the results with canaries behind them"""

    def __init__(self, P, cap):
        self.P, self.n = P, len(cap)
        self.page_off = np.zeros(self.n + 1, np.uint64)
        self.page_off[0] = FIRST_ENTRY
        self.page_off[1:] = FIRST_ENTRY + np.cumsum(np.array(cap, np.uint64))
        self.entries = int(self.page_off[self.n])
        self.file = np.full(GUARD + self.entries * P + GUARD, FILL, np.uint8)
        self.page_len, self.page_src = (np.full(self.entries + EXTRA, CANARY, np.uint32) for _ in range(2))
        self.n_pages, self.in_done = (np.full(self.n + EXTRA, CANARY, np.uint32) for _ in range(2))
        self.n_pages[:self.n] = 0
        self.in_done[:self.n] = 0

    def copy(self):
        t = Tab.__new__(Tab)
        t.P, t.n, t.entries = self.P, self.n, self.entries
        for name in ("page_off", "file", "page_len", "page_src", "n_pages", "in_done"):
            setattr(t, name, getattr(self, name).copy())
        return t

    def span(self, i):
        return int(self.page_off[i]), int(self.page_off[i + 1]) - int(self.page_off[i])

    def page(self, e, length=None):
        at = GUARD + e * self.P
        return self.file[at:at + (self.P if length is None else length)]

    def pages_of(self, i):
        first = int(self.page_off[i])
        return [(int(self.page_src[e]), self.page(e, int(self.page_len[e])).tobytes()) for e in range(first, first + int(self.n_pages[i]))]

    def tail(self, i):
        """(base, T) of a well-formed stream"""
        first, k = int(self.page_off[i]), int(self.n_pages[i])
        base = int(self.page_src[first + k - 1]) if k else 0
        return base, int(self.in_done[i]) - base

    def raw(self):
        from lz4_flex_amd import block
        return block.PagedStreams(page_size=self.P, pages=self.file[GUARD:GUARD + self.entries * self.P], page_off=self.page_off,
                                  page_len=self.page_len[:self.entries], page_src=self.page_src[:self.entries], n_pages=self.n_pages[:self.n],
                                  in_done=self.in_done[:self.n], status=np.zeros(self.n, np.int32))


def assert_untouched(before, after, i, what=""):
    first, room = before.span(i)
    room = max(room, 0)
    assert (after.n_pages[i], after.in_done[i]) == (before.n_pages[i], before.in_done[i]), (what, i)
    assert (after.page_len[first:first + room] == before.page_len[first:first + room]).all(), (what, i)
    assert (after.page_src[first:first + room] == before.page_src[first:first + room]).all(), (what, i)
    assert (after.page(first, room * before.P) == before.page(first, room * before.P)).all(), (what, i)


def _tails(tab, add_len, wmax):
    """T_i as far as the tables can be believed (hostile tables: clamped), 0 for a stream that gets nothing"""
    out = []
    for i in range(tab.n):
        first, room = tab.span(i)
        k, S = int(tab.n_pages[i]), int(tab.in_done[i])
        T = min(max(S - int(tab.page_src[first + k - 1]), 0), wmax) if 0 < k <= room else 0
        out.append(T if add_len[i] else 0)
    return out


def append(lib, tab, adds, mem, wmin=0, wmax=0, max_rounds=None, stage_cap=None):
    """one lz4flex_paged_append; tab is updated in place.  Returns (status, stage_off, tail_src, stage) -- stage None in MEM_HOST -- and checks
    the canaries and that entries in front of the reopened one and at or behind the new n_pages, and whole streams that got nothing,
    were not written"""
    from lz4_flex_amd import _lib
    n, P = tab.n, tab.P
    before = tab.copy()
    src, add_off = G.pack(adds, 3)
    add_len = np.array([len(a) for a in adds], np.uint32)
    wmax_r = M.windows_of(P, wmin, wmax)[1]
    tails = _tails(tab, add_len, wmax_r)
    if max_rounds is None:
        max_rounds = M.rounds_bound(max(t + int(a) for t, a in zip(tails, add_len)), P, wmin, wmax)
    status = np.full(n + EXTRA, CANARY, np.int32)
    stage_off, tail_src = np.full(n + EXTRA, CANARY64, np.uint64), np.full(n + EXTRA, CANARY, np.uint32)
    arrays = [src, add_off, add_len, tab.file, tab.page_off, tab.page_len, tab.page_src, tab.n_pages, tab.in_done, status, stage_off, tail_src]
    stage = None
    if mem == "host":
        p = [C.c_void_p(a.ctypes.data) for a in arrays]
        p[3] = C.c_void_p(tab.file.ctypes.data + GUARD)
        rc = lib.lz4flex_paged_append(None, *p[:3], n, P, wmin, wmax, max_rounds, *p[3:10], None, 0, p[10], p[11], None, 0, None, _lib.MEM_HOST, None)
        assert rc == 0, _lib.last_error()
    else:
        import torch
        t = [G._dev(a) for a in arrays]
        p = [C.c_void_p(x.data_ptr()) for x in t]
        p[3] = C.c_void_p(t[3].data_ptr() + GUARD)
        dev = t[0].device
        if stage_cap is None:
            stage_cap = int(lib.lz4flex_paged_append_stage_bound(int(add_len.sum()), n, wmax_r))      # always suffices
        d_stage = torch.full((GUARD + stage_cap + GUARD,), FILL, dtype=torch.uint8, device=dev)
        offered = sum(min(t_ + int(a), wmax_r) for t_, a in zip(tails, add_len) if a)
        scratch_cap = int(lib.lz4flex_compress_packed_scratch_bound(offered, n, 0))
        scratch = torch.empty(scratch_cap + 1, dtype=torch.uint8, device=dev)
        work = torch.empty(int(lib.lz4flex_paged_append_work_size(n)), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        rc = lib.lz4flex_paged_append(None, *p[:3], n, P, wmin, wmax, max_rounds, *p[3:10], C.c_void_p(d_stage.data_ptr() + GUARD), stage_cap,
                                      p[10], p[11], C.c_void_p(scratch.data_ptr()), scratch_cap, C.c_void_p(work.data_ptr()), _lib.MEM_DEVICE,
                                      C.c_void_p(stream.cuda_stream))
        assert rc == 0, _lib.last_error()
        stream.synchronize()
        tab.file = t[3].cpu().numpy()
        tab.page_len, tab.page_src, tab.n_pages, tab.in_done, tail_src = (t[j].cpu().numpy().view(np.uint32) for j in (5, 6, 7, 8, 11))
        status, stage_off = t[9].cpu().numpy(), t[10].cpu().numpy().view(np.uint64)
        h = d_stage.cpu().numpy()
        assert (h[:GUARD] == FILL).all() and (h[-GUARD:] == FILL).all(), "guard bytes around the stage were written"
        stage = h[GUARD:GUARD + stage_cap]
    assert (tab.file[:GUARD] == FILL).all() and (tab.file[-GUARD:] == FILL).all(), "guard bytes around the page file were written"
    assert (tab.page_len[tab.entries:] == CANARY).all() and (tab.page_src[tab.entries:] == CANARY).all(), "the tables were written past their end"
    for a, c in ((tab.n_pages, CANARY), (tab.in_done, CANARY), (status, CANARY), (tail_src, CANARY), (stage_off, CANARY64)):
        assert (a[n:] == c).all(), "results written past n"
    assert (tab.page_len[:FIRST_ENTRY] == CANARY).all() and (tab.page(0, FIRST_ENTRY * P) == FILL).all(), "entries of no stream were written"
    for i in range(n):
        first, room = before.span(i)
        k = int(before.n_pages[i])
        if not adds[i]:
            assert (int(status[i]), int(stage_off[i]), int(tail_src[i])) == (0, NO_STAGE, int(before.in_done[i])), i
        if not adds[i] or int(stage_off[i]) == NO_STAGE and mem == "device" or int(status[i]) == E_INVALID_ARG:
            assert_untouched(before, tab, i, "a stream that takes no part")
            continue
        k0, new_k = max(k - 1, 0), int(tab.n_pages[i])
        assert new_k <= room, i
        for a, b in ((tab.page_len, before.page_len), (tab.page_src, before.page_src)):
            assert (a[first:first + k0] == b[first:first + k0]).all(), ("entries in front of the reopened one", i)
            assert (a[first + new_k:first + room] == b[first + new_k:first + room]).all(), ("entries at or behind n_pages", i)
        assert (tab.page(first, k0 * P) == before.page(first, k0 * P)).all(), ("pages in front of the reopened one", i)
        assert mem == "host" or int(stage_off[i]) % 64 == 0
    return [int(v) for v in status[:n]], [int(v) for v in stage_off[:n]], [int(v) for v in tail_src[:n]], stage


def yardstick(lib, data, before, adds, dead, P, mem, **kw):
    """ONE lz4flex_compress_paged over tail ++ add, the tails from the source, dead streams empty, at the capacity behind the reopened entry"""
    V, cap = [], []
    for i, s in enumerate(data):
        base, T = before.tail(i)
        go = bool(adds[i]) and i not in dead
        assert not go or s[base + T:base + T + len(adds[i])] == adds[i]
        V.append(s[base:base + T + len(adds[i])] if go else b"")
        cap.append(before.span(i)[1] - max(int(before.n_pages[i]) - 1, 0) if go else 0)
    if "max_rounds" not in kw:
        kw["max_rounds"] = M.rounds_bound(max(len(v) for v in V), P, kw.get("wmin", 0), kw.get("wmax", 0))
    return G.run_paged(lib, V, P, cap, mem, **kw)[0]


def compare(tab, before, got_status, want, adds, dead, what):
    """the defining equality for every stream that went on"""
    n_pages, in_done, status, pages = want
    for i in range(tab.n):
        if not adds[i] or i in dead:
            continue
        base, _ = before.tail(i)
        k0 = max(int(before.n_pages[i]) - 1, 0)
        assert (int(tab.n_pages[i]) - k0, int(tab.in_done[i]) - base, got_status[i]) == (n_pages[i], in_done[i], status[i]), (what, i)
        got = [(pos - base, b) for pos, b in tab.pages_of(i)[k0:]]
        assert [pos for pos, _ in got] == [pos for pos, _ in pages[i]], (what, "page_src", i)
        assert [len(b) for _, b in got] == [len(b) for _, b in pages[i]], (what, "page_len", i)
        assert got == pages[i], (what, "page bytes", i)


def cuts(data):
    """a batch's mix: stream j stays fresh, is paged up to its last byte, to a third, or whole before the append under test"""
    return [(0, len(s) - 1, len(s) // 3, len(s))[(j + j // 14) % 4] if len(s) else 0 for j, s in enumerate(data)]     # (the cases come round every 14)


def two_steps(lib, data, P, mem, cap=None, **kw):
    """the tab after the first parts went in (itself an append to fresh streams, held to the yardstick), and the second parts"""
    cut = cuts(data) if len(data) > 1 else [len(data[0]) // 3]
    tab = Tab(P, [M.pages_bound(len(s), P) for s in data] if cap is None else cap)
    firsts = [s[:c] for s, c in zip(data, cut)]
    before = tab.copy()
    st, stage_off, tail_src, _ = append(lib, tab, firsts, mem, **kw)
    compare(tab, before, st, yardstick(lib, data, before, firsts, (), P, mem, **kw), firsts, (), "fresh")
    assert tail_src == [0] * len(data)
    return tab, [s[c:] for s, c in zip(data, cut)]


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("P,which", BATCHES, ids=["%d-%s" % b for b in BATCHES])
@pytest.mark.parametrize("mode,depth", MODES, ids=[m for m, _ in MODES])
def test_an_append_equals_one_paged_call_over_tail_and_add(lib, settings, mode, depth, P, which, mem):
    from lz4_flex_amd import block
    settings(mode, depth)
    data = G.batch(P, which)
    tab, adds = two_steps(lib, data, P, mem)
    if len(data) > 1:
        kinds = [(int(tab.n_pages[i]) == 0, len(a)) for i, a in enumerate(adds)]
        assert sum(1 for fresh, a in kinds if fresh and a) >= 5 and sum(1 for _, a in kinds if a == 0) >= 5          # fresh, nothing,
        assert sum(1 for fresh, a in kinds if not fresh and a == 1) >= 5                                           # one byte,
        assert sum(1 for fresh, a in kinds if not fresh and a > 3 * P) >= 2                                        # several pages' worth
    before = tab.copy()
    st, stage_off, tail_src, stage = append(lib, tab, adds, mem)
    want = yardstick(lib, data, before, adds, (), P, mem)
    compare(tab, before, st, want, adds, (), (mode, P, which, mem))
    assert st == [0] * len(data) and [int(v) for v in tab.in_done[:tab.n]] == [len(s) for s in data]
    assert tail_src == [before.tail(i)[0] if adds[i] else int(before.in_done[i]) for i in range(tab.n)]
    assert all(int(tab.n_pages[i]) <= M.pages_bound(len(s), P) for i, s in enumerate(data))
    if mem == "device":
        for i, a in enumerate(adds):                                              # the stage holds tail ++ add
            base = tail_src[i]
            assert not a or stage[stage_off[i]:stage_off[i] + len(data[i]) - base].tobytes() == data[i][base:], i
    else:
        assert stage_off == [NO_STAGE] * len(data)
    assert block.decompress_paged(tab.raw()) == data


@pytest.mark.parametrize("form", ["host", "device"])
def test_three_appends_and_the_read_side(lib, settings, form):
    """compress_paged, reserve_paged, then THREE appends through the Python forms -- the second and the third reopen a page that an
    append wrote after reopening one itself: decompress_paged and read_paged_ranges return the source, whole streams and ranges that
    cross a seam; every page but a stream's last holds at least Lfit(P) bytes and the pages bound holds after every append"""
    import torch
    from lz4_flex_amd import block
    settings("exact")
    P = 509
    data = G.batch(P, "n37")
    L = M.lfit_page(P)
    n = len(data)
    cut4 = [(0, len(s) // 4, len(s) // 2, 3 * len(s) // 4, len(s)) for s in data]
    parts = [[s[c[j]:c[j + 1]] for s, c in zip(data, cut4)] for j in range(4)]
    seams = [(c[2], c[3]) for c in cut4]                                          # both lie between two appends
    cap = [M.pages_bound(len(s), P) for s in data]
    dev = torch.device("cuda", 0)

    def up(part):
        src, off = G.pack(part, 0)
        return torch.from_numpy(src).to(dev), torch.from_numpy(off.astype(np.int64)), torch.tensor([len(x) for x in part], dtype=torch.int64)

    if form == "host":
        paged = block.reserve_paged(block.compress_paged(parts[0], P), cap)
        for j, part in enumerate(parts[1:]):
            paged = block.append_paged(paged, part)
            assert (paged.status == 0).all()
            assert all(int(k) <= M.pages_bound(c[j + 2], P) and int(d) == c[j + 2] for k, d, c in zip(paged.n_pages, paged.in_done, cut4)), j
        tables = paged
        back = block.decompress_paged(paged)
    else:
        paged = block.reserve_paged(block.compress_paged_device(*up(parts[0]), P), torch.tensor(cap))
        for j, part in enumerate(parts[1:]):
            paged, stage, stage_off, tail_src = block.append_paged_device(paged, *up(part))
            assert (paged.status.cpu().numpy() == 0).all()
            assert all(int(k) <= M.pages_bound(c[j + 2], P) and int(d) == c[j + 2]
                       for k, d, c in zip(paged.n_pages.cpu().numpy(), paged.in_done.cpu().numpy(), cut4)), j
        out, out_off, out_len, st = block.decompress_paged_device(paged)
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == 0).all()
        h = out.cpu().numpy()
        back = [h[int(o):int(o) + int(k)].tobytes() for o, k in zip(out_off.cpu().numpy(), out_len.cpu().numpy())]
        tables = block.PagedStreams(page_size=P, **{k: getattr(paged, k).cpu().numpy() for k in ("pages", "page_off", "page_len", "page_src",
                                                                                                 "n_pages", "in_done", "status")})
    assert back == data
    for i, s in enumerate(data):                                                  # the invariant behind both page bounds
        first, k = int(tables.page_off[i]), int(tables.n_pages[i])
        starts = [int(v) for v in tables.page_src[first:first + k]] + [len(s)]
        assert int(tables.in_done[i]) == len(s) and k <= M.pages_bound(len(s), P), i
        assert all(b - a >= L for a, b in zip(starts[:-2], starts[1:-1])), i
    sid, off, length = [], [], []
    for i, (s, (a, b)) in enumerate(zip(data, seams)):
        for r in ((0, 0xFFFFFFFF), (max(a - 5, 0), 11), (max(b - 3, 0), 700), (max(a - 1, 0), b - a + 2)):
            sid.append(i), off.append(r[0]), length.append(r[1])
    if form == "host":
        got, st = block.read_paged_ranges(paged, sid, off, length)
    else:
        out, out_off, out_len, st = block.read_paged_ranges_device(paged, sid, off, length)
        torch.cuda.synchronize()
        h, st = out.cpu().numpy(), st.cpu().numpy()
        got = [h[int(o):int(o) + int(k)].tobytes() for o, k in zip(out_off.cpu().numpy(), out_len.cpu().numpy())]
    assert (np.asarray(st) == 0).all()
    assert got == [data[i][o:o + k] for i, o, k in zip(sid, off, length)]


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("mode,depth", MODES[:2], ids=[m for m, _ in MODES[:2]])
def test_small_appends_behind_streams_that_get_nothing(lib, settings, mode, depth, mem):
    """the ordinary small append: every T + A is at most window_min, so round 1 offers every going stream whole and the scratch has no
    slack -- with idle streams and a contradicting table in front, whose empty windows take a scratch slot in every round all the same.
    Every going stream ends with status 0, in MEM_HOST too, where the library sizes the scratch itself"""
    from lz4_flex_amd import block
    settings(mode, depth)
    P = 64
    text = dict(G.K.streams(P, cut=G.CUT[P]))["text"]
    data = [text[40 * j:40 * j + 60 + j] for j in range(24)]
    firsts = [s[:50] for s in data]
    adds = [b"" if j < 9 or j % 5 == 0 else s[50:] for j, s in enumerate(data)]       # nine idle streams in front, more between
    tab = Tab(P, [3] * len(data))
    assert append(lib, tab, firsts, mem)[0] == [0] * len(data)
    spoilt = 9                                                                    # ... and a stream that is refused, in front as well
    tab.n_pages[spoilt] = 0
    assert adds[spoilt] and all(tab.tail(i)[1] + len(a) <= 4 * P for i, a in enumerate(adds) if i != spoilt)
    before = tab.copy()
    st, stage_off, tail_src, stage = append(lib, tab, adds, mem)
    assert st == [E_INVALID_ARG if i == spoilt else 0 for i in range(tab.n)], st
    compare(tab, before, st, yardstick(lib, data, before, adds, {spoilt}, P, mem), adds, {spoilt}, ("small appends", mode, mem))
    tab.n_pages[spoilt] = before.n_pages[spoilt] = 1
    assert block.decompress_paged(tab.raw()) == [s if a and i != spoilt else s[:50] for i, (s, a) in enumerate(zip(data, adds))]
    # the two-stream case as a caller writes it
    if mem == "host":
        paged = block.reserve_paged(block.compress_paged([b"abcdefgh" * 4, b"01234567" * 3], P), [2, 2])
        paged = block.append_paged(paged, [b"", b"0123456789"])
        assert paged.status.tolist() == [0, 0] and paged.in_done.tolist() == [32, 34]
        assert block.decompress_paged(paged) == [b"abcdefgh" * 4, b"01234567" * 3 + b"0123456789"]


def test_a_short_stage_refuses_the_later_streams(lib, settings):
    settings("exact")
    P = 64
    data = G.batch(P, "n37")
    tab, adds = two_steps(lib, data, P, "device")
    need = [(tab.tail(i)[1] + len(a) + 63) // 64 * 64 if a else 0 for i, a in enumerate(adds)]
    going = [i for i, a in enumerate(adds) if a]
    cutoff = going[len(going) // 2]
    stage_cap = sum(need[:cutoff + 1]) - 1                                        # the slot of `cutoff` ends one byte behind it
    dead = {i for i in going if sum(need[:i + 1]) > stage_cap}
    assert cutoff in dead and 3 <= len(dead) < len(going)
    before = tab.copy()
    st, stage_off, tail_src, stage = append(lib, tab, adds, "device", stage_cap=stage_cap)
    for i in dead:
        assert (st[i], stage_off[i], tail_src[i]) == (E_OUTPUT_TOO_SMALL, NO_STAGE, before.tail(i)[0]), i
        assert_untouched(before, tab, i, "refused")
    served = [i for i in going if i not in dead]
    assert [stage_off[i] for i in served] == [sum(need[:i]) for i in served]
    compare(tab, before, st, yardstick(lib, data, before, adds, dead, P, "device"), adds, dead, "short stage")
    assert [st[i] for i in served] == [0] * len(served)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_out_of_pages_and_out_of_rounds_lose_nothing(lib, settings, mem):
    from lz4_flex_amd import block
    settings("exact")
    P = 64
    data = G.batch(P, "n37")
    cut = cuts(data)
    k1 = G.run_paged(lib, [s[:c] for s, c in zip(data, cut)], P, [M.pages_bound(c, P) for c in cut], mem)[0][0]
    for name, cap, rounds in (("C == k", k1, None), ("max_rounds 0", None, 0), ("max_rounds 1", None, 1)):
        tab, adds = two_steps(lib, data, P, mem, cap=cap)
        assert cap is None or [int(v) for v in tab.n_pages[:tab.n]] == k1
        before = tab.copy()
        kw = {} if rounds is None else {"max_rounds": rounds}
        st, stage_off, tail_src, stage = append(lib, tab, adds, mem, **kw)
        compare(tab, before, st, yardstick(lib, data, before, adds, (), P, mem, **kw), adds, (), (name, mem))
        assert E_OUTPUT_TOO_SMALL in st and set(st) <= {0, E_OUTPUT_TOO_SMALL}, name
        if rounds == 0:
            assert all(s == E_OUTPUT_TOO_SMALL for s, a in zip(st, adds) if a)
        back = block.decompress_paged(tab.raw())
        for i, (s, a) in enumerate(zip(data, adds)):
            done = int(tab.in_done[i])
            assert back[i] == s[:done], (name, i)                                 # a valid prefix [0, in_done)
            if not a:
                continue
            assert tail_src[i] <= done <= len(s) and (done == len(s)) == (st[i] == 0), (name, i)
            if mem == "device":                                                   # the bytes not yet paged, at the documented place
                at = stage_off[i] + done - tail_src[i]
                assert stage[at:at + len(s) - done].tobytes() == s[done:], (name, i)
            else:
                assert stage_off[i] == NO_STAGE


@pytest.mark.parametrize("mem", ["host", "device"])
def test_hostile_tables_and_damaged_tail_pages(lib, settings, mem):
    """every contradiction of the rule's step 2 on a stream of its own, a tail page that does not decode and one that ends before the table
    says so: each leaves its stream untouched, the neighbours equal the yardstick with those streams empty"""
    from lz4_flex_amd import block
    settings("exact")
    P, wmin, wmax = 64, 64, 256
    data = G.batch(P, "n37")
    cut = [len(s) // 2 for s in data]
    tab = Tab(P, [M.pages_bound(len(s), P) + 1 for s in data])
    firsts = [s[:c] for s, c in zip(data, cut)]
    st, _, _, _ = append(lib, tab, firsts, mem, wmin=wmin, wmax=wmax)
    assert st == [0] * len(data)
    adds = [s[c:] for s, c in zip(data, cut)]
    victims = [i for i in range(tab.n - 1) if int(tab.n_pages[i]) >= 1 and adds[i]]
    assert len(victims) >= 12
    last = lambda i: int(tab.page_off[i]) + int(tab.n_pages[i]) - 1               # noqa: E731
    want_st = {}
    v = iter(victims)

    def spoil(code, change, fits=lambda i: True):
        i = next(j for j in v if fits(j))
        change(i)
        want_st[i] = code

    spoil(E_INVALID_ARG, lambda i: tab.n_pages.__setitem__(i, tab.span(i)[1] + 1))                                 # k > C
    spoil(E_INVALID_ARG, lambda i: tab.n_pages.__setitem__(i, 0))                                                  # k == 0 with S != 0
    spoil(E_INVALID_ARG, lambda i: tab.page_len.__setitem__(last(i), 0))
    spoil(E_INVALID_ARG, lambda i: tab.page_len.__setitem__(last(i), P + 1))
    spoil(E_INVALID_ARG, lambda i: tab.page_src.__setitem__(last(i), int(tab.in_done[i])))                         # page_src[e] >= S
    spoil(E_INVALID_ARG, lambda i: tab.page_src.__setitem__(last(i), 0xFFFFFFF0))
    spoil(E_INVALID_ARG, lambda i: tab.in_done.__setitem__(i, int(tab.page_src[last(i)]) + wmax + 1))              # T > window_max
    def huge(i):                                                                                                   # S + A > 2^32 - 1
        tab.in_done[i] = 0xFFFFFFFF - len(adds[i]) + 1
        tab.page_src[last(i)] = int(tab.in_done[i]) - 5
    spoil(E_INVALID_ARG, huge)
    def damaged(i):                                                                                                # a match 65 535 bytes back
        e = last(i)
        tab.page(e)[:3] = (0x00, 0xFF, 0xFF)
        tab.page_len[e] = max(int(tab.page_len[e]), 8)
    spoil(None, damaged)
    broken = max(want_st)
    _, T = tab.tail(broken)
    block_bytes = tab.page(last(broken), int(tab.page_len[last(broken)])).copy()
    got_len, code = block.decompress_batch_partial(block_bytes, [0], [len(block_bytes)], np.zeros(T + 64, np.uint8), [0], [T])[:2]
    assert int(code[0]) != 0                                                       # the decoder's own code for that page
    want_st[broken] = int(code[0])
    spoil(E_EXPECTED_ANOTHER_BYTE, lambda i: tab.in_done.__setitem__(i, int(tab.in_done[i]) + 3),                  # the page ends before S
          fits=lambda i: tab.tail(i)[1] + 3 <= wmax)
    down = tab.n - 1                                                                                               # page_off counting down
    assert adds[down]
    tab.page_off[tab.n] = tab.page_off[down] - 1
    want_st[down] = E_INVALID_ARG
    dead = set(want_st)
    before = tab.copy()
    st, stage_off, tail_src, stage = append(lib, tab, adds, mem, wmin=wmin, wmax=wmax)
    for i, code in want_st.items():
        assert st[i] == code, (i, st[i], code)
        assert_untouched(before, tab, i, "hostile")
        assert code not in (E_INVALID_ARG,) or stage_off[i] == NO_STAGE
    # the neighbours: the yardstick over the sound streams (the tails from the source), the spoilt ones empty
    sound = before.copy()
    V, cap = [], []
    for i, s in enumerate(data):
        go = bool(adds[i]) and i not in dead
        base, T = sound.tail(i) if go else (0, 0)
        V.append(s[base:] if go else b"")
        cap.append(sound.span(i)[1] - max(int(sound.n_pages[i]) - 1, 0) if go else 0)
    rounds = M.rounds_bound(max(len(x) for x in V), P, wmin, wmax)
    want = G.run_paged(lib, V, P, cap, mem, wmin=wmin, wmax=wmax, max_rounds=rounds)[0]
    compare(tab, before, st, want, adds, dead, ("neighbours", mem))
    assert all(st[i] == 0 and int(tab.in_done[i]) == len(data[i]) for i in range(tab.n) if adds[i] and i not in dead)
