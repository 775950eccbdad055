"""CPU tests of the paged rule (lz4flex_compress_paged, include/lz4flex_amd.h): tests/paged_model.py over the oracle's exact encoder
(oracle_api.compress) and the fit rule (tests/fit_model.py) -- every page decodes to exactly its slice, the slices tile the stream, the
bounds hold and are met where the header says so, a run of zeros retries up to window_max and leaves its pages underfilled -- and the
library's side that needs no device: the two bound functions equal the model's, every argument check answers before a context is looked
at.  No compute calls."""
import ctypes as C
import os

import pytest

import oracle_api as O
import paged_cases as K
import paged_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lz4flex_amd.h")


def oracle_round(windows):
    return [(O.compress(w), M.OK) for w in windows]


@pytest.fixture(scope="module")
def runs():
    """{P: (names, streams, the model's result with capacities of exactly the bound)}, computed once"""
    out = {}
    for P in K.PAGE_SIZES:
        cases = K.streams(P)
        data = [s for _, s in cases]
        cap = [M.pages_bound(len(s), P) for s in data]
        out[P] = ([nm for nm, _ in cases], data, M.run(data, P, cap, M.by_encoder(oracle_round)))
    return out


@pytest.mark.parametrize("P", K.PAGE_SIZES)
def test_pages_decode_to_their_slices_and_tile_the_stream(runs, P):
    names, data, r = runs[P]
    L = M.lfit_page(P)
    assert r.status == [M.OK] * len(data)
    assert r.in_done == [len(s) for s in data]
    for nm, s, pages, k in zip(names, data, r.pages, r.n_pages):
        assert len(pages) == k and (k == 0) == (len(s) == 0), nm
        ends = [pos for pos, _ in pages[1:]] + [len(s)]
        at = 0
        for j, ((pos, block), end) in enumerate(zip(pages, ends)):
            assert pos == at and end > pos, (nm, j)                              # the slices tile the stream, every page holds something
            assert len(block) <= P, (nm, j, len(block))
            assert O.decompress(block, end - pos) == ("ok", s[pos:end]), (nm, j)
            if j + 1 < k:
                assert end - pos >= L, (nm, j, end - pos)                        # a page with more to come used at least Lfit(P)
            at = end
        assert at == len(s), nm


@pytest.mark.parametrize("P", K.PAGE_SIZES)
def test_the_bounds_hold(runs, P):
    names, data, r = runs[P]
    for nm, s, k, retries in zip(names, data, r.n_pages, r.retries):
        assert k <= M.pages_bound(len(s), P), nm
        assert k + retries <= M.rounds_bound(len(s), P), nm
    assert r.rounds <= M.rounds_bound(max(len(s) for s in data), P)
    assert r.rounds == max(k + t for k, t in zip(r.n_pages, r.retries))
    total = sum(len(s) for s in data)
    assert total <= r.offered                                                # (every byte is offered at least once)


@pytest.mark.parametrize("P", K.PAGE_SIZES)
def test_the_incompressible_stream_meets_the_page_bound_exactly(runs, P):
    names, data, r = runs[P]
    i = names.index("noise")
    L = M.lfit_page(P)
    assert len(data[i]) == 3 * P + 7 and r.n_pages[i] == M.pages_bound(3 * P + 7, P) == -(-(3 * P + 7) // L)
    assert [len(b) for _, b in r.pages[i][:-1]] == [P] * (r.n_pages[i] - 1)        # every page but the last is full: L literals
    assert [pos for pos, _ in r.pages[i]] == [j * L for j in range(r.n_pages[i])]
    # one page less: OUTPUT_TOO_SMALL, the pages so far valid
    cap = [M.pages_bound(len(s), P) for s in data]
    cap[i] -= 1
    short = M.run(data, P, cap, M.by_encoder(oracle_round))
    assert short.status[i] == M.E_OUTPUT_TOO_SMALL and short.n_pages[i] == cap[i] and short.in_done[i] == cap[i] * L
    assert short.pages[i] == r.pages[i][:cap[i]]
    assert [x for j, x in enumerate(short.status) if j != i] == [M.OK] * (len(data) - 1)
    # the edges of one page of literals
    a, b = names.index("lfit"), names.index("lfit+1")
    assert (r.n_pages[a], len(r.pages[a][0][1])) == (1, P) and r.n_pages[b] == 2 and r.pages[b][1][0] == L


@pytest.mark.parametrize("P", K.PAGE_SIZES)
def test_the_zero_stream_retries_up_to_window_max_and_underfills(runs, P):
    """a window of zeros fits a page whole whatever its length: W doubles until window_max, and a page then holds window_max bytes (or
    what the fit rule's clipped match reaches, where even that block is longer than a page) in a fraction of P"""
    names, data, r = runs[P]
    i = names.index("zeros")
    wmin, wmax = M.windows_of(P)
    assert (wmin, wmax) == (4 * P, 65536)
    whole = len(O.compress(bytes(wmax)))
    if whole <= P:
        assert r.retries[i] == M.doublings(wmin, wmax) and r.n_pages[i] == 1 and len(r.pages[i][0][1]) == whole
    # a stream longer than window_max: every page holds window_max bytes and is all but empty
    small = 4 * P
    z = M.run([bytes(8 * small)], P, [M.pages_bound(8 * small, P)], M.by_encoder(oracle_round), window_min=P, window_max=small)
    if len(O.compress(bytes(small))) <= P:
        assert z.retries == [2] and z.n_pages == [8] and z.status == [M.OK]
        assert [pos for pos, _ in z.pages[0]] == [j * small for j in range(8)]
        assert all(len(b) < P // 2 for _, b in z.pages[0])
    assert z.rounds <= M.rounds_bound(8 * small, P, P, small)
    assert M.replay_offered(8 * small, [pos for pos, _ in z.pages[0]], z.in_done[0], P, P, small) == z.offered


@pytest.mark.parametrize("P", K.PAGE_SIZES)
def test_replaying_the_results_gives_the_offered_bytes(runs, P):
    names, data, r = runs[P]
    got = sum(M.replay_offered(len(s), [pos for pos, _ in pages], done, P) for s, pages, done in zip(data, r.pages, r.in_done))
    assert got == r.offered


def test_rounds_run_out_and_capacity_zero():
    P = 64
    data = [K.streams(P)[-1][1][:1000], b"", b"abc"]
    full = M.run(data, P, [M.pages_bound(len(s), P) for s in data], M.by_encoder(oracle_round))
    assert full.status == [0, 0, 0] and full.n_pages[1:] == [0, 1] and full.rounds == full.n_pages[0] + full.retries[0]
    short = M.run(data, P, [M.pages_bound(len(s), P) for s in data], M.by_encoder(oracle_round), max_rounds=full.rounds - 1)
    assert short.status == [M.E_OUTPUT_TOO_SMALL, 0, 0] and short.n_pages[0] == full.n_pages[0] - 1 < M.pages_bound(1000, P)
    assert short.pages[0] == full.pages[0][:-1] and short.in_done[0] == full.pages[0][-1][0]
    none = M.run(data, P, [0, 0, 0], M.by_encoder(oracle_round))
    assert none.status == [M.E_OUTPUT_TOO_SMALL, 0, M.E_OUTPUT_TOO_SMALL] and none.n_pages == [0, 0, 0] and none.rounds == 0
    failing = M.run(data, P, [20, 0, 1], lambda w, c: [(b"", 0, 5)] * 3)
    assert failing.status == [5, 0, 5] and failing.n_pages == [0, 0, 0]


# ---- the library's side that needs no device -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from lz4_flex_amd import _lib, build
    build.build()
    return _lib.load()


def test_the_bound_functions_equal_the_model(lib):
    lens = [0, 1, 61, 62, 63, 64, 65, 4095, 4096, 65535, 65536, 1 << 20, (1 << 31) + 5, 0xFFFFFFFF]
    pages = [64, 65, 79, 80, 81, 272, 273, 509, 4096, 65536, (4 << 20) - 1, 4 << 20]
    for P in pages:
        L = M.lfit_page(P)
        assert 1 + (0 if L < 15 else 1 + (L - 15) // 255) + L <= P < 2 + (0 if L + 1 < 15 else 1 + (L + 1 - 15) // 255) + L, P
        for n in lens + [L - 1, L, L + 1, 3 * P + 7]:
            assert lib.lz4flex_paged_pages_bound(n, P) == M.pages_bound(n, P), (n, P)
            for wmin, wmax in ((0, 0), (P, P), (P, 0), (0, 1 << 31), (P, 3 * P + 1), (4 * P, 1 << 31)):
                assert lib.lz4flex_paged_rounds_bound(n, P, wmin, wmax) == M.rounds_bound(n, P, wmin, wmax), (n, P, wmin, wmax)
    for P in (0, 1, 63, (4 << 20) + 1, 0xFFFFFFFF):
        assert lib.lz4flex_paged_pages_bound(1000, P) == 0 == M.pages_bound(1000, P)
        assert lib.lz4flex_paged_rounds_bound(1000, P, 0, 0) == 0 == M.rounds_bound(1000, P)
    for wmin, wmax in ((63, 0), (64, 63), (128, 127), (0, 255), (64, (1 << 31) + 1), ((1 << 31) + 1, 0)):
        assert lib.lz4flex_paged_rounds_bound(1000, 64, wmin, wmax) == 0 == M.rounds_bound(1000, 64, wmin, wmax), (wmin, wmax)
    assert M.rounds_bound(4096, 64) == 67 + 8 and M.pages_bound(65536, 4096) == 17
    for n in (0, 1, 37, 1024, 1025, 100000):
        assert lib.lz4flex_compress_paged_work_size(n) >= lib.lz4flex_compress_fit_work_size(n) + 44 * n
        assert lib.lz4flex_compress_paged_work_size(n) % 8 == 0


def _args():
    """a valid 1-stream call as ctypes arrays (host memory; a device pointer is never followed by an argument check)"""
    return dict(src=C.create_string_buffer(b"hello, hello, hello", 32), in_off=(C.c_uint64 * 1)(0), in_len=(C.c_uint32 * 1)(19),
                out=C.create_string_buffer(b"\xC5" * 128, 128), page_off=(C.c_uint64 * 2)(0, 2), page_len=(C.c_uint32 * 2)(7, 7),
                page_src=(C.c_uint32 * 2)(7, 7), n_pages=(C.c_uint32 * 1)(7), in_done=(C.c_uint32 * 1)(7), status=(C.c_int32 * 1)(7),
                scratch=C.create_string_buffer(256), work=C.create_string_buffer(8192))


def _paged(lib, a, n=1, mem=0, P=64, wmin=0, wmax=0, rounds=4, **over):
    a = dict(a, **over)
    return lib.lz4flex_compress_paged(None, a["src"], a["in_off"], a["in_len"], n, P, wmin, wmax, rounds, a["out"], a["page_off"], a["page_len"],
                                      a["page_src"], a["n_pages"], a["in_done"], a["status"], a["scratch"], 256, a["work"], mem, None)


ARRAYS = ("in_off", "in_len", "page_off", "page_len", "page_src", "n_pages", "in_done", "status")


def _untouched(a):
    return (a["page_len"][:], a["page_src"][:], a["n_pages"][0], a["in_done"][0], a["status"][0], a["out"].raw) == \
        ([7, 7], [7, 7], 7, 7, 7, b"\xC5" * 128)


def test_argument_checks_need_no_device(lib):
    from lz4_flex_amd import _lib
    INV = -_lib.E_INVALID_ARG
    a = _args()
    HOST, DEV, BIG, CHAINED = _lib.MEM_HOST, _lib.MEM_DEVICE, _lib.MEM_BIG_BLOCKS, _lib.MEM_CHAINED
    for mem in (HOST, DEV, HOST | BIG, DEV | BIG):
        for name in ARRAYS:
            assert _paged(lib, a, mem=mem, **{name: None}) == INV, name
        for P in (0, 1, 63, (4 << 20) + 1, 0xFFFFFFFF):
            assert _paged(lib, a, mem=mem, P=P) == INV and _paged(lib, a, mem=mem, P=P, n=0) == INV, P
        for wmin, wmax in ((63, 0), (64, 63), (128, 127), (0, 255), (64, (1 << 31) + 1), ((1 << 31) + 1, 0)):
            assert _paged(lib, a, mem=mem, wmin=wmin, wmax=wmax) == INV, (wmin, wmax)
    for mem in (7, HOST | CHAINED, DEV | CHAINED, DEV | CHAINED | BIG, 0x1001):
        assert _paged(lib, a, mem=mem) == INV, hex(mem)
    assert _paged(lib, a, n=0, mem=9) == INV                               # a bad mem_kind is refused even when there is nothing to do
    assert _paged(lib, a, mem=DEV, scratch=None) == INV and _paged(lib, a, mem=DEV | BIG, work=None) == INV
    assert _paged(lib, a, mem=HOST, page_off=(C.c_uint64 * 2)(2, 0)) == INV  # the entries count up
    assert _untouched(a)


def test_nothing_to_do_and_no_device(lib):
    from lz4_flex_amd import _lib, block
    a = _args()
    HOST, DEV, BIG = _lib.MEM_HOST, _lib.MEM_DEVICE, _lib.MEM_BIG_BLOCKS
    for mem in (HOST, DEV, HOST | BIG, DEV | BIG):
        assert _paged(lib, a, n=0, mem=mem) == 0
        assert _paged(lib, a, n=0, mem=mem, scratch=None, work=None, **{k: None for k in ARRAYS}) == 0
        assert _paged(lib, a, n=0, mem=mem, wmin=64, wmax=1 << 31, rounds=0) == 0
    if lib.lz4flex_device_count() == 0:
        NODEV = -_lib.E_NO_DEVICE
        assert _paged(lib, a) == NODEV and _paged(lib, a, mem=HOST | BIG) == NODEV and _paged(lib, a, scratch=None, work=None) == NODEV
        assert _untouched(a)
        with pytest.raises(block.DeviceError):
            block.compress_paged([b"hello, hello, hello"], 64)
    assert block.paged_pages_bound(4096, 64) == 67 and block.paged_rounds_bound(4096, 64) == 75


def test_declared_exported_bound_and_documented(lib):
    import re
    import subprocess
    from lz4_flex_amd import _lib, block, build
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(lz4flex_[a-z0-9_]+)\s*\(", src))
    exported = set(re.findall(r" T (lz4flex_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", build.LIB]).decode()))
    note = text[text.index("The round of this header:"):text.index("int lz4flex_abi_version(void);")]
    for name in ("lz4flex_compress_paged", "lz4flex_compress_paged_work_size", "lz4flex_paged_pages_bound", "lz4flex_paged_rounds_bound"):
        assert name in declared and name in exported and name in _lib.SIGNATURES and name in note, name
    assert len(_lib.SIGNATURES["lz4flex_compress_paged"][1]) == 21
    assert lib.lz4flex_abi_version() == 8
    for name in ("compress_paged", "compress_paged_device", "decompress_paged", "decompress_paged_device"):
        assert callable(getattr(block, name)), name
    assert b"paged_step_kernel" in open(build.LIB, "rb").read()
    for line in ("`pos = 0`, `W = window_min`, `k = 0`", "`w = min(W, in_len - pos)`", "`used == w`, `pos + w < in_len` and `W < window_max`",
                 "`W = min(2 * W, window_max)`", "`e = page_off[i] + k`", "`page_len[e] = out_len`, `page_src[e] = pos`", "`out_base + e * P`",
                 "`pos += used`, `k += 1`", "`ceil(in_len / Lfit(page_size, infinity))`", "`64 <= page_size <= 4 MiB`",
                 "`page_size <= window_min <= window_max <= 2^31`", "`window_max = max(window_min, 65536)`",
                 "table entries at or behind n_pages[i] stay untouched", "The arguments are checked before a context or a device is looked at"):
        assert line in text, line
