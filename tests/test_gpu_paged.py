"""GPU tests of the paged streams (lz4flex_compress_paged, lz4_paged.hip): the device loop equals, byte for byte and entry for entry, the
loop a caller could write before it existed -- one lz4flex_compress_batch_fit per round over the same n windows, the rule applied in Python
(tests/paged_model.py) -- for batches of 1 and of 37 streams, MEM_HOST and MEM_DEVICE, "compress_mode" 0, 1 and 2; in mode 1 it also
equals the model over the oracle's encoder.  The page table decodes with one lz4flex_decompress_batch; nothing outside the committed
pages' entries, the page file and the n results is written."""
import ctypes as C

import numpy as np
import pytest

import oracle_api as O
import paged_cases as K
import paged_model as M

pytestmark = pytest.mark.gpu

GUARD, FILL, CANARY, EXTRA = 64, 0xC5, 0x5A5A5A5A, 3
FIRST_ENTRY = 2                                            # page_off[0]: the table and the page file need not start at entry 0
MODES = [("fast", None), ("exact", None), ("high", 4)]
CUT = {64: 4096, 509: 20 * 1024, 4096: 20 * 1024}          # the text and JSON streams: at most about 70 rounds per page size
BATCHES = [(64, "n37"), (509, "n37"), (4096, "n37"), (64, "n1:json"), (64, "n1:noise"), (64, "n1:zeros"), (64, "n1:len13"), (64, "n1:len0")]


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

    def choose(mode, depth=None, serial=0):
        block.set_compress_mode(mode)
        if depth:
            block.set_compress_depth(depth)
        assert lib.lz4flex_set_tuning(None, b"fit_serial", serial) == 0
    yield choose
    block.set_compress_mode("fast")
    block.set_compress_depth(16)
    assert lib.lz4flex_set_tuning(None, b"fit_serial", 0) == 0


_batches = {}


def batch(P, which):
    """the streams of a batch: "n37" = the cases of tests/paged_cases.py taken round and round, "n1:<name>" = one of them alone"""
    if (P, which) not in _batches:
        cases = K.streams(P, cut=CUT[P])
        _batches[P, which] = [cases[(5 * j) % len(cases)][1] for j in range(37)] if which == "n37" else [dict(cases)[which.split(":")[1]]]
    return _batches[P, which]


def pack(parts, gap):
    offs, at = [], 1
    for p in parts:
        offs.append(at)
        at += len(p) + gap
    buf = np.full(at + 16, 0x77, np.uint8)
    for o, p in zip(offs, parts):
        buf[o:o + len(p)] = np.frombuffer(p, np.uint8)
    return buf, np.array(offs, np.uint64)


def fit_round(windows, caps):
    """the yardstick's round: ONE lz4flex_compress_batch_fit (it exists without lz4flex_compress_paged and has its own tests) over the n
    windows of the round, the settings as they are"""
    from lz4_flex_amd import block
    n, P = len(windows), max(max(caps), 1)
    src, off = pack(windows, 0)
    out = np.zeros(n * P, np.uint8)
    out_off = np.arange(n, dtype=np.uint64) * P
    out_len, used, st = block.compress_batch_fit(src, off, [len(w) for w in windows], out, out_off, caps)
    return [(out[int(o):int(o) + int(ln)].tobytes(), int(u), int(s)) for o, ln, u, s in zip(out_off, out_len, used, st)]


_yard = {}


def yardstick(key, data, P, cap, **kw):
    """the host loop with the rule in Python, once per (settings, batch, arguments); the result is shared and left unchanged"""
    if key not in _yard:
        _yard[key] = M.run(data, P, cap, fit_round, **kw)
    return _yard[key]


def result_of(r):
    return (r.n_pages, r.in_done, r.status, r.pages)


def _dev(a):
    import torch
    v = a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a
    return torch.from_numpy(np.array(v)).to(torch.device("cuda", 0))


def run_paged(lib, data, P, cap, mem, wmin=0, wmax=0, max_rounds=None):
    """one lz4flex_compress_paged; returns (n_pages, in_done, status, pages) in the model's form plus the PagedStreams of the raw arrays, and
    checks that nothing but the page file, committed table entries and the n results was written"""
    from lz4_flex_amd import _lib, block
    n = len(data)
    src, in_off = pack(data, 3)
    in_len = np.array([len(s) for s in data], np.uint32)
    page_off = np.zeros(n + 1, np.uint64)
    page_off[0] = FIRST_ENTRY
    page_off[1:] = FIRST_ENTRY + np.cumsum(np.array(cap, np.uint64))
    entries = int(page_off[n])
    if max_rounds is None:
        max_rounds = M.rounds_bound(int(in_len.max()), P, wmin, wmax)
    file = np.full(GUARD + entries * P + GUARD, FILL, np.uint8)
    page_len, page_src = np.full(entries + EXTRA, CANARY, np.uint32), np.full(entries + EXTRA, CANARY, np.uint32)
    n_pages, in_done, status = (np.full(n + EXTRA, CANARY, dt) for dt in (np.uint32, np.uint32, np.int32))
    arrays = [src, in_off, in_len, file, page_off, page_len, page_src, n_pages, in_done, status]
    if mem == "host":
        p = [C.c_void_p(a.ctypes.data) for a in arrays]
        p[3] = C.c_void_p(file.ctypes.data + GUARD)
        rc = lib.lz4flex_compress_paged(None, *p[:3], n, P, wmin, wmax, max_rounds, *p[3:], None, 0, None, _lib.MEM_HOST, None)
        assert rc == 0, _lib.last_error()
    else:
        import torch
        t = [_dev(a) for a in arrays]
        p = [C.c_void_p(x.data_ptr()) for x in t]
        p[3] = C.c_void_p(t[3].data_ptr() + GUARD)
        offered = int(np.minimum(in_len, M.windows_of(P, wmin, wmax)[1]).sum())
        scratch_cap = int(lib.lz4flex_compress_packed_scratch_bound(offered, n, 0))
        scratch = torch.empty(scratch_cap + 1, dtype=torch.uint8, device=t[0].device)
        work = torch.empty(int(lib.lz4flex_compress_paged_work_size(n)), dtype=torch.uint8, device=t[0].device)
        stream = torch.cuda.current_stream(t[0].device)
        rc = lib.lz4flex_compress_paged(None, *p[:3], n, P, wmin, wmax, max_rounds, *p[3:], C.c_void_p(scratch.data_ptr()), scratch_cap,
                                        C.c_void_p(work.data_ptr()), _lib.MEM_DEVICE, C.c_void_p(stream.cuda_stream))
        assert rc == 0, _lib.last_error()
        stream.synchronize()
        file = t[3].cpu().numpy()
        page_len, page_src, n_pages, in_done = (t[j].cpu().numpy().view(np.uint32) for j in (5, 6, 7, 8))
        status = t[9].cpu().numpy()
    assert (file[:GUARD] == FILL).all() and (file[-GUARD:] == FILL).all(), "guard bytes around the page file were written"
    assert (n_pages[n:] == CANARY).all() and (in_done[n:] == CANARY).all() and (status[n:] == CANARY).all(), "results written past n"
    committed = np.zeros(entries + EXTRA, bool)
    pages = []
    for i in range(n):
        first, k = int(page_off[i]), int(n_pages[i])
        assert k <= cap[i], (i, k, cap[i])
        committed[first:first + k] = True
        assert (page_len[first:first + k] <= P).all(), i
        pages.append([(int(page_src[e]), file[GUARD + e * P:GUARD + e * P + int(page_len[e])].tobytes()) for e in range(first, first + k)])
    assert (page_len[~committed] == CANARY).all() and (page_src[~committed] == CANARY).all(), "table entries at or behind n_pages were written"
    raw = block.PagedStreams(page_size=P, pages=file[GUARD:GUARD + entries * P], page_off=page_off, page_len=page_len[:entries],
                             page_src=page_src[:entries], n_pages=n_pages[:n], in_done=in_done[:n], status=status[:n])
    return ([int(v) for v in n_pages[:n]], [int(v) for v in in_done[:n]], [int(v) for v in status[:n]], pages), raw


def compare(got, want, what):
    for name, g, w in zip(("n_pages", "in_done", "status"), got, want):
        assert g == w, (what, name, [(i, a, b) for i, (a, b) in enumerate(zip(g, w)) if a != b][:8])
    for i, (g, w) in enumerate(zip(got[3], want[3])):
        assert [pos for pos, _ in g] == [pos for pos, _ in w], (what, "page_src", i)
        assert [len(b) for _, b in g] == [len(b) for _, b in w], (what, "page_len", i)
        assert g == w, (what, "page bytes", i)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("P,which", BATCHES, ids=["%d-%s" % b for b in BATCHES])
@pytest.mark.parametrize("mode,depth", MODES, ids=[m for m, _ in MODES])
def test_the_device_loop_equals_the_host_loop(lib, settings, mode, depth, P, which, mem):
    from lz4_flex_amd import block
    settings(mode, depth)
    data = batch(P, which)
    cap = [M.pages_bound(len(s), P) for s in data]                            # capacities of exactly the bound
    want = yardstick((mode, P, which), data, P, cap)
    assert want.status == [0] * len(data) and want.in_done == [len(s) for s in data]
    assert want.rounds <= 80, want.rounds
    # MEM_DEVICE enqueues exactly max_rounds rounds: two more than the data needs change nothing
    got, raw = run_paged(lib, data, P, cap, mem, max_rounds=want.rounds + 2 if mem == "device" else None)
    compare(got, result_of(want), (mode, P, which, mem))
    if mode == "exact":
        oracle = M.run(data, P, cap, M.by_encoder(lambda ws: [(O.compress(w), 0) for w in ws]))
        compare(got, result_of(oracle), (mode, P, which, mem, "oracle"))
    assert block.decompress_paged(raw) == data                                # ONE lz4flex_decompress_batch over the page table


def test_fit_serial_gives_the_same_results(lib, settings):
    P, which = 64, "n37"
    data = batch(P, which)
    cap = [M.pages_bound(len(s), P) for s in data]
    settings("exact")
    want = yardstick(("exact", P, which), data, P, cap)
    settings("exact", serial=1)
    for mem in ("host", "device"):
        got, _ = run_paged(lib, data, P, cap, mem, max_rounds=want.rounds)
        compare(got, result_of(want), ("fit_serial", mem))


@pytest.mark.parametrize("mem", ["host", "device"])
def test_out_of_pages(lib, settings, mem):
    """the bound - 1 on the incompressible stream, and capacity 0: OUTPUT_TOO_SMALL, the pages so far valid, the other streams as they were"""
    from lz4_flex_amd import block
    settings("exact")
    P, which = 64, "n37"
    data = batch(P, which)
    L = M.lfit_page(P)
    cap = [M.pages_bound(len(s), P) for s in data]
    full = yardstick(("exact", P, which), data, P, cap)
    noise = [i for i, s in enumerate(data) if len(s) == 3 * P + 7]
    assert noise and all(full.n_pages[i] == cap[i] for i in noise)          # (it meets the bound exactly)
    i, z = noise[0], noise[-1]
    assert i != z
    cap[i] -= 1
    cap[z] = 0
    want = yardstick(("exact", P, which, "short"), data, P, cap)
    got, raw = run_paged(lib, data, P, cap, mem, max_rounds=full.rounds)
    compare(got, result_of(want), ("out of pages", mem))
    assert got[2][i] == got[2][z] == M.E_OUTPUT_TOO_SMALL and got[0][i] == cap[i] and got[1][i] == cap[i] * L
    assert got[3][i] == full.pages[i][:cap[i]] and (got[0][z], got[1][z]) == (0, 0)
    assert [s for j, s in enumerate(got[2]) if j not in (i, z)] == [0] * (len(data) - 2)
    back = block.decompress_paged(raw)
    assert back == [s[:got[1][j]] for j, s in enumerate(data)]


@pytest.mark.parametrize("mem", ["host", "device"])
def test_out_of_rounds(lib, settings, mem):
    """max_rounds one short of what the slowest stream needs: it ends with OUTPUT_TOO_SMALL, n_pages below its capacity, its pages valid"""
    from lz4_flex_amd import block
    settings("exact")
    P, which = 64, "n37"
    data = batch(P, which)
    cap = [M.pages_bound(len(s), P) for s in data]
    full = yardstick(("exact", P, which), data, P, cap)
    want = yardstick(("exact", P, which, "rounds"), data, P, cap, max_rounds=full.rounds - 1)
    got, raw = run_paged(lib, data, P, cap, mem, max_rounds=full.rounds - 1)
    compare(got, result_of(want), ("out of rounds", mem))
    late = [j for j in range(len(data)) if full.n_pages[j] + full.retries[j] == full.rounds]
    assert late and all(got[2][j] == M.E_OUTPUT_TOO_SMALL and got[0][j] == full.n_pages[j] - 1 < cap[j] for j in late)
    assert all(got[3][j] == full.pages[j][:-1] for j in late)
    assert [got[2][j] for j in range(len(data)) if j not in late] == [0] * (len(data) - len(late))
    assert block.decompress_paged(raw) == [s[:got[1][j]] for j, s in enumerate(data)]
    # no rounds at all: every stream that has bytes ends at once
    got, _ = run_paged(lib, data, P, cap, mem, max_rounds=0)
    assert got[0] == [0] * len(data) and got[1] == [0] * len(data)
    assert got[2] == [M.E_OUTPUT_TOO_SMALL if len(s) else 0 for s in data]


@pytest.mark.parametrize("mem", ["host", "device"])
def test_explicit_windows(lib, settings, mem):
    """window_min = window_max = page_size (no retries, the least work per page) and a window_max that is no power-of-two multiple"""
    settings("exact")
    P, which = 509, "n37"
    data = batch(P, which)
    cap = [M.pages_bound(len(s), P) for s in data]
    for wmin, wmax in ((P, P), (P, 3 * P + 1)):
        want = yardstick(("exact", P, which, wmin, wmax), data, P, cap, window_min=wmin, window_max=wmax)
        assert want.status == [0] * len(data) and want.rounds <= M.rounds_bound(max(len(s) for s in data), P, wmin, wmax)
        got, _ = run_paged(lib, data, P, cap, mem, wmin=wmin, wmax=wmax, max_rounds=want.rounds)
        compare(got, result_of(want), ("windows", wmin, wmax, mem))


def test_python_forms_round_trip(lib, settings):
    import torch
    from lz4_flex_amd import block
    settings("fast")
    P = 509
    data = batch(P, "n37")
    res = block.compress_paged(data, P)
    assert (res.status == 0).all() and [int(v) for v in res.in_done] == [len(s) for s in data]
    assert all(int(k) <= M.pages_bound(len(s), P) for k, s in zip(res.n_pages, data))
    assert block.decompress_paged(res) == data
    dev = torch.device("cuda", 0)
    src, in_off = pack(data, 0)
    in_len = torch.tensor([len(s) for s in data], dtype=torch.int64)
    d = block.compress_paged_device(torch.from_numpy(src).to(dev), torch.from_numpy(in_off.astype(np.int64)), in_len, P)
    torch.cuda.synchronize()
    assert d.page_off.cpu().numpy().astype(np.uint64).tolist() == res.page_off.tolist()
    for name in ("n_pages", "in_done", "status", "page_len", "page_src"):
        a, b = getattr(d, name).cpu().numpy(), getattr(res, name)
        keep = np.ones(a.size, bool)
        if name in ("page_len", "page_src"):                                  # (entries at or behind n_pages: whatever they were)
            keep[:] = False
            for i in range(len(data)):
                keep[int(res.page_off[i]):int(res.page_off[i]) + int(res.n_pages[i])] = True
        assert (a.astype(np.int64)[keep] == b.astype(np.int64)[keep]).all(), name
    out, out_off, out_len, st = block.decompress_paged_device(d)
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (st.cpu().numpy() == 0).all()
    assert [h[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(out_off.cpu().numpy(), out_len.cpu().numpy())] == data
    # a capacity of one page per stream: the streams that need more end with OUTPUT_TOO_SMALL and decode as far as they got
    one = block.compress_paged_device(torch.from_numpy(src).to(dev), torch.from_numpy(in_off.astype(np.int64)), in_len, P,
                                      page_cap=torch.ones(len(data), dtype=torch.int64), max_rounds=8)
    out, out_off, out_len, st = block.decompress_paged_device(one)
    torch.cuda.synchronize()
    h, done = out.cpu().numpy(), one.in_done.cpu().numpy()
    assert (st.cpu().numpy() == 0).all() and (one.n_pages.cpu().numpy() == [1 if s else 0 for s in data]).all()
    assert (one.status.cpu().numpy() == [0 if int(u) == len(s) else M.E_OUTPUT_TOO_SMALL for u, s in zip(done, data)]).all()
    assert [h[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(out_off.cpu().numpy(), out_len.cpu().numpy())] == \
        [s[:int(u)] for u, s in zip(done, data)]
    assert any(int(u) < len(s) for u, s in zip(done, data))
