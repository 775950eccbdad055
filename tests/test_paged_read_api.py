"""CPU tests of the side of lz4flex_paged_read_ranges that needs no device: the pages bound equals the model's, the work size is monotone
and aligned, every argument check answers before a context or a device is looked at and in the header's order, the symbols are declared,
exported and bound, and without a device a well-formed call says so.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

import paged_read_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lz4flex_amd.h")
NAMES = ("lz4flex_paged_read_ranges", "lz4flex_paged_read_work_size", "lz4flex_paged_range_pages_bound")


@pytest.fixture(scope="module")
def lib():
    from lz4_flex_amd import _lib, build
    build.build()
    return _lib.load()


def test_the_pages_bound_equals_the_model(lib):
    from lz4_flex_amd import block
    for P in (64, 509, 4096):
        L = R.lfit_page(P)
        for n in (0, 1, 2, L + 1, L + 2, 2 * L + 2, 0xFFFFFFFF):
            assert lib.lz4flex_paged_range_pages_bound(n, P) == R.pages_bound(n, P) == block.paged_range_pages_bound(n, P), (n, P)
        assert [R.pages_bound(n, P) for n in (0, 1, 2, L + 1, L + 2, 2 * L + 2)] == [0, 1, 2, 2, 3, 4]
    assert R.pages_bound(0xFFFFFFFF, 64) == 2 + (0xFFFFFFFF - 2) // 62
    for P in (0, 63, (4 << 20) + 1, 0xFFFFFFFF):
        assert lib.lz4flex_paged_range_pages_bound(1000, P) == 0 == R.pages_bound(1000, P), P
    assert lib.lz4flex_paged_range_pages_bound(1000, 4 << 20) == 2


def test_the_work_size_is_monotone_and_aligned(lib):
    sizes = (0, 1, 2, 37, 255, 256, 1024, 1025, 65536, 1 << 20)
    for m in sizes:
        row = [lib.lz4flex_paged_read_work_size(m, t) for t in sizes]
        assert row == sorted(row) and all(v % 8 == 0 for v in row), m
        col = [lib.lz4flex_paged_read_work_size(t, m) for t in sizes]
        assert col == sorted(col), m
        # a record, two sizes, two sums, two batches' items and results and a gather per range; a batch's items and results per slot
        assert lib.lz4flex_paged_read_work_size(m, m) >= (48 + 4 * 8 + 4 * 8 + 5 * 4) * m + (2 * 8 + 4 * 4) * m
    assert lib.lz4flex_paged_read_work_size(1 << 20, 1 << 22) > lib.lz4flex_paged_read_work_size(1 << 20, 1 << 20)


def _args():
    """a well-formed call over one stream of two pages as ctypes arrays (host memory; a device pointer is never followed by an argument
    check), every result array filled with 7"""
    return dict(pages=C.create_string_buffer(b"\x10a" + bytes(62) + b"\x10b" + bytes(62), 128), page_off=(C.c_uint64 * 2)(0, 2),
                page_len=(C.c_uint32 * 2)(2, 2), page_src=(C.c_uint32 * 2)(0, 1), n_pages=(C.c_uint32 * 1)(2), in_done=(C.c_uint32 * 1)(2),
                range_stream=(C.c_uint32 * 1)(0), range_off=(C.c_uint32 * 1)(0), range_len=(C.c_uint32 * 1)(2), out=C.create_string_buffer(b"\xC5" * 16, 16),
                out_off=(C.c_uint64 * 1)(4), out_len=(C.c_uint32 * 1)(7), status=(C.c_int32 * 1)(7), scratch=C.create_string_buffer(256),
                work=C.create_string_buffer(16384))


ARRAYS = ("page_off", "page_len", "page_src", "n_pages", "in_done", "range_stream", "range_off", "range_len", "out_off", "out_len", "status")


def _read(lib, a, m=1, mem=0, P=64, n=1, max_items=2, scratch_cap=256, **over):
    a = dict(a, **over)
    return lib.lz4flex_paged_read_ranges(None, a["pages"], P, a["page_off"], a["page_len"], a["page_src"], a["n_pages"], a["in_done"], n,
                                         a["range_stream"], a["range_off"], a["range_len"], m, a["out"], a["out_off"], a["out_len"], a["status"],
                                         max_items, a["scratch"], scratch_cap, a["work"], mem, None)


def _untouched(a):
    return (a["out_len"][0], a["status"][0], a["out"].raw) == (7, 7, b"\xC5" * 16)


def test_argument_checks_need_no_device_and_keep_their_order(lib):
    from lz4_flex_amd import _lib
    INV = -_lib.E_INVALID_ARG
    HOST, DEV, BIG, CHAINED = _lib.MEM_HOST, _lib.MEM_DEVICE, _lib.MEM_BIG_BLOCKS, _lib.MEM_CHAINED
    a = _args()
    for mem in (HOST, DEV, HOST | BIG, DEV | BIG):
        for name in ARRAYS:
            assert _read(lib, a, mem=mem, **{name: None}) == INV, name
            assert _read(lib, a, mem=mem, m=0, **{name: None}) == 0, name          # nothing to do: the arrays are not looked at
        for P in (0, 1, 63, (4 << 20) + 1, 0xFFFFFFFF):
            assert _read(lib, a, mem=mem, P=P) == INV and _read(lib, a, mem=mem, P=P, m=0) == INV, P      # ... the page size is
        assert _read(lib, a, mem=mem, m=0) == 0 and _read(lib, a, mem=mem, m=0, P=4 << 20, n=0, max_items=0, scratch_cap=0) == 0
        assert _read(lib, a, mem=mem, m=0, scratch=None, work=None, pages=None, out=None, **{k: None for k in ARRAYS}) == 0
    for mem in (7, HOST | CHAINED, DEV | CHAINED, DEV | CHAINED | BIG, 0x1001):
        assert _read(lib, a, mem=mem) == INV and _read(lib, a, mem=mem, m=0) == INV, hex(mem)             # ... and the mem_kind
    assert _read(lib, a, mem=DEV, work=None) == INV and _read(lib, a, mem=DEV | BIG, scratch=None) == INV
    assert _read(lib, a, mem=DEV, work=None, m=0) == 0
    assert _untouched(a)


def test_no_device_is_said_so(lib):
    from lz4_flex_amd import _lib, block
    import numpy as np
    a = _args()
    if lib.lz4flex_device_count() == 0:
        NODEV = -_lib.E_NO_DEVICE
        assert _read(lib, a) == NODEV and _read(lib, a, mem=_lib.MEM_HOST | _lib.MEM_BIG_BLOCKS) == NODEV
        assert _read(lib, a, mem=_lib.MEM_DEVICE) == NODEV and _read(lib, a, mem=_lib.MEM_DEVICE, scratch=None, scratch_cap=0) == NODEV
        assert _read(lib, a, scratch=None, work=None) == NODEV                                            # HOST: both are ignored
        assert _untouched(a)
        paged = block.PagedStreams(page_size=64, pages=np.frombuffer(a["pages"].raw, np.uint8), page_off=np.array([0, 2], np.uint64),
                                   page_len=np.array([2, 2], np.uint32), page_src=np.array([0, 1], np.uint32), n_pages=np.array([2], np.uint32),
                                   in_done=np.array([2], np.uint32), status=np.zeros(1, np.int32))
        with pytest.raises(block.DeviceError):
            block.read_paged_ranges(paged, [0], [0], [2])
    assert block.read_paged_ranges(block.PagedStreams(page_size=64, pages=np.zeros(0, np.uint8), page_off=np.zeros(1, np.uint64),
                                                      page_len=np.zeros(0, np.uint32), page_src=np.zeros(0, np.uint32), n_pages=np.zeros(0, np.uint32),
                                                      in_done=np.zeros(0, np.uint32), status=np.zeros(0, np.int32)), [], [], [])[0] == []


def test_declared_exported_bound_and_documented(lib):
    from lz4_flex_amd import _lib, block, build
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(lz4flex_[a-z0-9_]+)\s*\(", src))
    exported = set(re.findall(r" T (lz4flex_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", build.LIB]).decode()))
    note = text[text.index("The round of this header:"):text.index("int lz4flex_abi_version(void);")]
    for name in NAMES:
        assert name in declared and name in exported and name in _lib.SIGNATURES and name in note, name
    assert len(_lib.SIGNATURES["lz4flex_paged_read_ranges"][1]) == 23
    assert lib.lz4flex_abi_version() == 8
    for name in ("paged_range_pages_bound", "read_paged_ranges", "read_paged_ranges_device", "decompress_paged", "decompress_paged_device"):
        assert callable(getattr(block, name)), name
    binary = open(build.LIB, "rb").read()
    for kernel in (b"paged_read_locate_kernel", b"paged_read_check_kernel", b"paged_read_emit_kernel", b"paged_read_verdict_kernel"):
        assert kernel in binary, kernel
    for line in ("`k = min(n_pages[i], C)`", "`out_len[r] = min(range_len[r], S - range_off[r])`", "`page_src[first + j] <= pos`",
                 "`head_bytes = min(range end, page end) - page start`", "`slot_r + nb_r <= max_items`", "`head_off_r + head_bytes_r <= scratch_cap`",
                 "`2 + (L - 2) / Lfit(P, infinity)`", "`m * roundup64(window_max)`", "LZ4FLEX_E_EXPECTED_ANOTHER_BYTE if the page decodes without an error",
                 "checked before a context or a device is looked at"):
        assert line in text, line
