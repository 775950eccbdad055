"""CPU tests of the side of lz4flex_paged_append that needs no device: the stage bound and the work size against the model, every argument
check answers before a context or a device is looked at and in the order of lz4flex_compress_paged, the symbols are declared, exported
and bound, without a device a well-formed call says so, the Python wrappers refuse what they must, and reserve_paged moves numpy tables.
No compute calls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import paged_append_model as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lz4flex_amd.h")
NAMES = ("lz4flex_paged_append", "lz4flex_paged_append_work_size", "lz4flex_paged_append_stage_bound")


@pytest.fixture(scope="module")
def lib():
    from lz4_flex_amd import _lib, build
    build.build()
    return _lib.load()


def test_the_stage_bound_and_the_work_size(lib):
    from lz4_flex_amd import block
    for total in (0, 1, 255, 1 << 20, (1 << 40) + 7):
        for n in (0, 1, 37, 65536, 0xFFFFFFFF):
            for wmax in (0, 64, 65, 509, 65536, 65537, 1 << 31):
                want = total + n * ((wmax or 65536) + 63)
                assert lib.lz4flex_paged_append_stage_bound(total, n, wmax) == A.stage_bound(total, n, wmax) == want, (total, n, wmax)
                assert wmax == 0 or block.paged_append_stage_bound(total, n, 64, 64, wmax) == want
            # the Python form resolves the windows as the entry does: the default window_max is max(4 P, 65536), whatever P is
            for P, wmin, resolved in ((64, 0, 65536), (16384, 0, 65536), (16385, 0, 4 * 16385), (4 << 20, 0, 16 << 20), (64, 1 << 20, 1 << 20)):
                assert block.paged_append_stage_bound(total, n, P, wmin) == total + n * (resolved + 63), (total, n, P, wmin)
            for wmax in (1, 63, (1 << 31) + 1, 0xFFFFFFFF):                      # no window of the paged entries: refused
                assert lib.lz4flex_paged_append_stage_bound(total, n, wmax) == 0 == A.stage_bound(total, n, wmax), (total, n, wmax)
    sizes = [lib.lz4flex_paged_append_work_size(n) for n in (0, 1, 2, 37, 255, 256, 1024, 1025, 65536, 1 << 20)]
    assert sizes == sorted(sizes) and all(v % 8 == 0 for v in sizes)
    for n in (0, 1, 37, 1024, 1025, 100000):
        # the rounds' own area, a record, the slot size and its sum, five offsets and six words per stream
        assert lib.lz4flex_paged_append_work_size(n) >= lib.lz4flex_compress_paged_work_size(n) + (40 + 2 * 8 + 5 * 8 + 6 * 4) * n


def _args():
    """a well-formed call over one stream of one page as ctypes arrays (host memory; a device pointer is never followed by an argument
    check), every result array filled with 7"""
    return dict(add=C.create_string_buffer(b"hello, hello", 16), add_off=(C.c_uint64 * 1)(0), add_len=(C.c_uint32 * 1)(12),
                pages=C.create_string_buffer(b"\x10a" + bytes(62) + b"\xC5" * 64, 128), page_off=(C.c_uint64 * 2)(0, 2),
                page_len=(C.c_uint32 * 2)(2, 7), page_src=(C.c_uint32 * 2)(0, 7), n_pages=(C.c_uint32 * 1)(1), in_done=(C.c_uint32 * 1)(1),
                status=(C.c_int32 * 1)(7), stage=C.create_string_buffer(b"\xC5" * 256, 256), stage_off=(C.c_uint64 * 1)(7),
                tail_src=(C.c_uint32 * 1)(7), scratch=C.create_string_buffer(256), work=C.create_string_buffer(16384))


ARRAYS = ("add_off", "add_len", "page_off", "page_len", "page_src", "n_pages", "in_done", "status", "stage_off", "tail_src")


def _append(lib, a, n=1, mem=0, P=64, wmin=0, wmax=0, rounds=4, stage_cap=256, **over):
    a = dict(a, **over)
    return lib.lz4flex_paged_append(None, a["add"], a["add_off"], a["add_len"], n, P, wmin, wmax, rounds, a["pages"], a["page_off"], a["page_len"],
                                    a["page_src"], a["n_pages"], a["in_done"], a["status"], a["stage"], stage_cap, a["stage_off"], a["tail_src"],
                                    a["scratch"], 256, a["work"], mem, None)


def _untouched(a):
    return (a["page_len"][:], a["page_src"][:], a["n_pages"][0], a["in_done"][0], a["status"][0], a["stage_off"][0], a["tail_src"][0],
            a["pages"].raw, a["stage"].raw) == ([2, 7], [0, 7], 1, 1, 7, 7, 7, b"\x10a" + bytes(62) + b"\xC5" * 64, b"\xC5" * 256)


def test_argument_checks_need_no_device_and_keep_their_order(lib):
    from lz4_flex_amd import _lib
    INV = -_lib.E_INVALID_ARG
    HOST, DEV, BIG, CHAINED = _lib.MEM_HOST, _lib.MEM_DEVICE, _lib.MEM_BIG_BLOCKS, _lib.MEM_CHAINED
    a = _args()
    for mem in (HOST, DEV, HOST | BIG, DEV | BIG):
        for name in ARRAYS:
            assert _append(lib, a, mem=mem, **{name: None}) == INV, name
            assert _append(lib, a, mem=mem, n=0, **{name: None}) == 0, name          # nothing to do: the arrays are not looked at
        for P in (0, 1, 63, (4 << 20) + 1, 0xFFFFFFFF):                          # the page size and the windows come first ...
            assert _append(lib, a, mem=mem, P=P) == INV and _append(lib, a, mem=mem, P=P, n=0) == INV, P
        for wmin, wmax in ((63, 0), (64, 63), (128, 127), (0, 255), (64, (1 << 31) + 1), ((1 << 31) + 1, 0)):
            assert _append(lib, a, mem=mem, wmin=wmin, wmax=wmax) == INV and _append(lib, a, mem=mem, wmin=wmin, wmax=wmax, n=0) == INV
        assert _append(lib, a, mem=mem, n=0) == 0 and _append(lib, a, mem=mem, n=0, wmin=64, wmax=1 << 31, rounds=0, stage_cap=0) == 0
        assert _append(lib, a, mem=mem, n=0, add=None, pages=None, stage=None, scratch=None, work=None, **{k: None for k in ARRAYS}) == 0
    for mem in (7, HOST | CHAINED, DEV | CHAINED, DEV | CHAINED | BIG, 0x1001):      # ... then the mem_kind, even with nothing to do
        assert _append(lib, a, mem=mem) == INV and _append(lib, a, mem=mem, n=0) == INV, hex(mem)
    for missing in ("work", "scratch", "stage"):                                  # DEVICE: the three buffers the caller brings
        assert _append(lib, a, mem=DEV, **{missing: None}) == INV and _append(lib, a, mem=DEV | BIG, **{missing: None}) == INV, missing
        assert _append(lib, a, mem=DEV, n=0, **{missing: None}) == 0
    assert _untouched(a)


def test_no_device_is_said_so(lib):
    from lz4_flex_amd import _lib, block
    a = _args()
    if lib.lz4flex_device_count() == 0:
        NODEV = -_lib.E_NO_DEVICE
        assert _append(lib, a) == NODEV and _append(lib, a, mem=_lib.MEM_HOST | _lib.MEM_BIG_BLOCKS) == NODEV
        assert _append(lib, a, mem=_lib.MEM_DEVICE) == NODEV and _append(lib, a, mem=_lib.MEM_DEVICE | _lib.MEM_BIG_BLOCKS) == NODEV
        assert _append(lib, a, stage=None, scratch=None, work=None) == NODEV       # HOST: the three are ignored
        assert _untouched(a)
        with pytest.raises(block.DeviceError):
            block.append_paged(_one_stream(), [b"more"])
    assert block.append_paged(_no_streams(), []).n_pages.size == 0               # n == 0 returns 0: no device is looked at


def _one_stream():
    from lz4_flex_amd import block
    pages = np.zeros(128, np.uint8)
    pages[:2] = (0x10, ord("a"))
    return block.PagedStreams(page_size=64, pages=pages, page_off=np.array([0, 2], np.uint64), page_len=np.array([2, 0], np.uint32),
                              page_src=np.array([0, 0], np.uint32), n_pages=np.array([1], np.uint32), in_done=np.array([1], np.uint32),
                              status=np.zeros(1, np.int32))


def _no_streams():
    from lz4_flex_amd import block
    return block.PagedStreams(page_size=64, pages=np.zeros(0, np.uint8), page_off=np.zeros(1, np.uint64), page_len=np.zeros(0, np.uint32),
                              page_src=np.zeros(0, np.uint32), n_pages=np.zeros(0, np.uint32), in_done=np.zeros(0, np.uint32),
                              status=np.zeros(0, np.int32))


def test_the_python_wrappers_refuse_what_they_must():
    from lz4_flex_amd import block
    with pytest.raises(ValueError):
        block.append_paged(_one_stream(), [b"a", b"b"])                          # one bytes-like object per stream
    with pytest.raises(ValueError):
        block.append_paged(_one_stream(), [])
    wrong = _one_stream()
    wrong.n_pages = wrong.n_pages.astype(np.int64)                               # the call updates the table in place: no converted copy
    with pytest.raises(ValueError):
        block.append_paged(wrong, [b"a"])
    wrong = _one_stream()
    wrong.pages = np.zeros(256, np.uint8)[::2]
    with pytest.raises(ValueError):
        block.append_paged(wrong, [b"a"])
    with pytest.raises(block.DeviceError):
        block.append_paged(_one_stream(), [b"a"], window_min=63)                 # the library's own check, before a device is looked at
    for cap in ([0], [1, 1], []):
        with pytest.raises(ValueError):
            block.reserve_paged(_one_stream(), cap)


def test_reserve_paged_moves_numpy_tables():
    from lz4_flex_amd import block
    P = 64
    rng = np.random.default_rng(5)
    n_pages = np.array([2, 0, 3, 1], np.uint32)
    page_off = np.array([3, 5, 5, 9, 10], np.uint64)                             # stream 2 has a free entry, entries 0 .. 2 belong to nobody
    entries = 10
    pages = rng.integers(0, 256, entries * P, dtype=np.uint8)
    page_len = rng.integers(1, P + 1, entries).astype(np.uint32)
    page_src = rng.integers(0, 1000, entries).astype(np.uint32)
    old = block.PagedStreams(page_size=P, pages=pages, page_off=page_off, page_len=page_len, page_src=page_src, n_pages=n_pages,
                             in_done=np.array([100, 0, 300, 50], np.uint32), status=np.array([0, 0, 1, 0], np.int32))
    keep = [a.copy() for a in (pages, page_off, page_len, page_src, n_pages)]
    cap = [4, 2, 3, 6]
    new = block.reserve_paged(old, cap)
    assert new.page_off.tolist() == [0, 4, 6, 9, 15] and new.page_off.dtype == np.uint64 and new.pages.size == 15 * P
    assert new.page_len.dtype == new.page_src.dtype == np.uint32 and new.page_len.size == 15
    for i in range(4):
        for j in range(int(n_pages[i])):
            e, f = int(page_off[i]) + j, int(new.page_off[i]) + j
            assert (new.page_len[f], new.page_src[f]) == (page_len[e], page_src[e]), (i, j)
            assert (new.pages[f * P:(f + 1) * P] == pages[e * P:(e + 1) * P]).all(), (i, j)
    for name in ("n_pages", "in_done", "status"):
        assert (getattr(new, name) == getattr(old, name)).all() and getattr(new, name) is not getattr(old, name)
    assert all((a == b).all() for a, b in zip(keep, (pages, page_off, page_len, page_src, n_pages)))      # the old streams are not changed
    same = block.reserve_paged(new, cap)
    assert all((getattr(same, k) == getattr(new, k)).all() for k in ("pages", "page_off", "page_len", "page_src"))
    assert block.reserve_paged(_no_streams(), []).page_off.tolist() == [0]


def test_declared_exported_bound_and_documented(lib):
    from lz4_flex_amd import _lib, block, build
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(lz4flex_[a-z0-9_]+)\s*\(", src))
    exported = set(re.findall(r" T (lz4flex_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", build.LIB]).decode()))
    note = text[text.index("The round of this header:"):text.index("int lz4flex_abi_version(void);")]
    for name in NAMES:
        assert name in declared and name in exported and name in _lib.SIGNATURES and name in note, name
    assert len(_lib.SIGNATURES["lz4flex_paged_append"][1]) == 25
    assert lib.lz4flex_abi_version() == 8                                         # new symbols only
    for name in ("append_paged", "append_paged_device", "paged_append_stage_bound", "reserve_paged"):
        assert callable(getattr(block, name)), name
    binary = open(build.LIB, "rb").read()
    for kernel in (b"paged_append_locate_kernel", b"paged_append_emit_kernel", b"paged_append_resume_kernel", b"paged_step_kernel"):
        assert kernel in binary, kernel
    for line in ("`first = page_off[i]`, `C = page_off[i+1] - first`, `k = n_pages[i]`, `S = in_done[i]`", "`status[i] = 0`, `stage_off[i] = ~0`, `tail_src[i] = S`",
                 "`k == 0` with `S != 0`", "`T = S - page_src[e] > window_max`", "`S + A > 2^32 - 1`", "`roundup64(T + A)`",
                 "`sum_add_len + n * (window_max + 63)`", "LZ4FLEX_E_EXPECTED_ANOTHER_BYTE", "`V = tail ++ add`",
                 "`W = window_min`, `pos = base` and page index `k - 1`", "`stage + stage_off[i] + (in_done[i] - tail_src[i])`",
                 "`C - (k - 1)`", "before a context or a device is looked at", "skipping the reopen when the tail page is known to be full"):
        assert line in text, line
