"""CPU test of the packed batch entries (lz4flex_decompress_batch_packed, lz4flex_compress_batch_packed and their two helpers): declared,
exported and bound; the ABI number stays; every argument check answers before a context or a device is looked at; the scratch bound holds
for any split of the input.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lz4flex_amd.h")
ENTRIES = ["lz4flex_decompress_batch_packed", "lz4flex_compress_batch_packed", "lz4flex_packed_work_size",
           "lz4flex_compress_packed_scratch_bound"]


@pytest.fixture(scope="module")
def lib():
    from lz4_flex_amd import _lib, build
    build.build()
    return _lib.load()


def test_declared_exported_and_bound(lib):
    from lz4_flex_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(lz4flex_[a-z0-9_]+)\s*\(", src))
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB]).decode()
    exported = set(re.findall(r" T (lz4flex_[a-z0-9_]+)", out))
    for name in ENTRIES:
        assert name in declared and name in exported and name in _lib.SIGNATURES, name
    for name, value in (("LZ4FLEX_SIZES_PREPENDED", 0), ("LZ4FLEX_SIZES_GIVEN", 1), ("LZ4FLEX_SIZES_SCAN", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), src), name
    assert (_lib.SIZES_PREPENDED, _lib.SIZES_GIVEN, _lib.SIZES_SCAN) == (0, 1, 2)
    assert lib.lz4flex_abi_version() == 8


def _args():
    """a valid 1-block batch as ctypes arrays (host memory; a device pointer is never followed by an argument check)"""
    return dict(src=C.create_string_buffer(bytes([1, 0, 0, 0, 0x10, 0x61]), 16), in_off=(C.c_uint64 * 1)(0), in_len=(C.c_uint32 * 1)(6),
                sizes=(C.c_uint32 * 1)(1), out=C.create_string_buffer(256), out_off=(C.c_uint64 * 2)(7, 7), out_cap=(C.c_uint32 * 1)(7),
                out_len=(C.c_uint32 * 1)(7), status=(C.c_int32 * 1)(7), detail=(C.c_uint64 * 2)(7, 7), work=C.create_string_buffer(4096),
                scratch=C.create_string_buffer(256))


def _decode(lib, a, n=1, mode=0, align=1, mem=0, **over):
    a = dict(a, **over)
    return lib.lz4flex_decompress_batch_packed(None, a["src"], a["in_off"], a["in_len"], n, mode, a["sizes"], a["out"], 256, align, a["out_off"],
                                               a["out_cap"], a["out_len"], a["status"], a["detail"], a["work"], mem, None)


def _compress(lib, a, n=1, prepend=1, align=1, mem=0, scratch_cap=256, **over):
    a = dict(a, **over)
    return lib.lz4flex_compress_batch_packed(None, a["src"], a["in_off"], a["in_len"], n, prepend, a["scratch"], scratch_cap, a["out"], 256,
                                             align, a["out_off"], a["out_len"], a["status"], a["work"], mem, None)


def test_argument_checks_need_no_device(lib):
    from lz4_flex_amd import _lib
    INV = -_lib.E_INVALID_ARG
    a = _args()
    HOST, DEV = _lib.MEM_HOST, _lib.MEM_DEVICE
    for mem in (HOST, DEV):
        for name in ("in_off", "in_len", "out_off", "out_cap", "out_len", "status"):
            assert _decode(lib, a, mem=mem, **{name: None}) == INV, ("decode", name)
        for name in ("in_off", "in_len", "out_off", "out_len", "status"):
            assert _compress(lib, a, mem=mem, **{name: None}) == INV, ("compress", name)
        assert _decode(lib, a, mode=_lib.SIZES_GIVEN, mem=mem, sizes=None) == INV
        for mode in (-1, 3, 99):
            assert _decode(lib, a, mode=mode, mem=mem) == INV, mode
        for align in (0, 3, 12, 24, 257, 512, 0x80000000):
            assert _decode(lib, a, align=align, mem=mem) == INV, align
            assert _compress(lib, a, align=align, mem=mem) == INV, align
    assert _decode(lib, a, mem=DEV, work=None) == INV
    assert _compress(lib, a, mem=DEV, work=None) == INV
    for mem in (7, HOST | _lib.MEM_CHAINED, DEV | _lib.MEM_CHAINED, DEV | _lib.MEM_CHAINED | _lib.MEM_BIG_BLOCKS, 0x1001):
        assert _decode(lib, a, mem=mem) == INV, hex(mem)
        assert _compress(lib, a, mem=mem) == INV, hex(mem)
    # a host batch's lengths are visible: scratch_cap below the slots (get_maximum_output_size(6) + 4 = 30)
    assert _compress(lib, a, scratch_cap=29) == INV
    # the bad scalar arguments are refused even when there is nothing to do
    assert _decode(lib, a, n=0, mode=5) == INV and _decode(lib, a, n=0, align=3) == INV and _compress(lib, a, n=0, mem=9) == INV
    # nothing of the results was touched
    assert (a["out_off"][0], a["out_cap"][0], a["out_len"][0], a["status"][0]) == (7, 7, 7, 7)


def test_nothing_to_do_and_no_device(lib):
    from lz4_flex_amd import _lib
    a = _args()
    for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE, _lib.MEM_HOST | _lib.MEM_BIG_BLOCKS, _lib.MEM_DEVICE | _lib.MEM_BIG_BLOCKS):
        for mode in (0, 1, 2):
            assert _decode(lib, a, n=0, mode=mode, mem=mem) == 0
            assert _decode(lib, a, n=0, mode=mode, mem=mem, in_off=None, work=None, sizes=None) == 0
        assert _compress(lib, a, n=0, mem=mem) == 0 and _compress(lib, a, n=0, mem=mem, prepend=0, work=None, scratch_cap=0) == 0
    if lib.lz4flex_device_count() == 0:
        NODEV = -_lib.E_NO_DEVICE
        for mode in (0, 1, 2):
            assert _decode(lib, a, mode=mode) == NODEV and _decode(lib, a, mode=mode, align=256, mem=_lib.MEM_HOST | _lib.MEM_BIG_BLOCKS) == NODEV
        assert _compress(lib, a) == NODEV and _compress(lib, a, prepend=0, scratch_cap=26, align=16) == NODEV
        assert (a["out_off"][0], a["out_len"][0], a["status"][0]) == (7, 7, 7)
        from lz4_flex_amd import block
        with pytest.raises(block.DeviceError):
            block.decompress_batch_packed(np.frombuffer(bytes([1, 0, 0, 0, 0x10, 0x61]), np.uint8), [0], [6], np.zeros(16, np.uint8))
        with pytest.raises(block.DeviceError):
            block.compress_batch_packed(np.frombuffer(b"no gpu, no codec", np.uint8), [0], [16], np.zeros(64, np.uint8))


def test_scratch_bound_holds_for_every_split(lib):
    max_out = lib.lz4flex_get_maximum_output_size
    rnd = np.random.default_rng(12)
    splits = [[0], [0] * 17, [1], [9] * 9, [99, 1], [65536] * 4, [70000, 0, 3, 4096, 4095, 11], [0xFFFFFFFF], [0xFFFFFFFF, 0xFFFFFFFF, 5],
              [1] * 1000, list(rnd.integers(0, 200, 777)), list(rnd.integers(0, 70001, 300)), list(rnd.integers(0, 1 << 24, 40))]
    for lens in splits:
        total, n = int(sum(int(v) for v in lens)), len(lens)
        for p in (0, 1):
            need = sum(int(max_out(int(v))) + 4 * p for v in lens)
            got = int(lib.lz4flex_compress_packed_scratch_bound(total, n, p))
            assert got >= need, (lens[:5], p, got, need)
            assert got <= need + n, (lens[:5], p, got, need)        # (the rounding of n divisions at most: the bound is not wasteful)
    assert lib.lz4flex_compress_packed_scratch_bound(0, 0, 1) == 0


def test_work_size_grows_with_the_batch(lib):
    sizes = [int(lib.lz4flex_packed_work_size(n)) for n in (0, 1, 1024, 1025, 65536, 1 << 20, 0xFFFFFFFF)]
    assert sizes == sorted(sizes) and sizes[1] > 0
    assert 32 * 65536 <= sizes[4] <= 33 * 65536 + 4096          # three arrays of u64, two of u32, the tile sums
    assert sizes[-1] > 32 * 0xFFFFFFFF                            # no 32-bit arithmetic on the way


def test_packed_scan_tile_is_a_known_key(lib):
    from lz4_flex_amd import _lib
    assert '"packed_scan_tile"' in open(HEADER).read()
    have = lib.lz4flex_device_count() > 0
    v = lib.lz4flex_get_tuning(None, b"packed_scan_tile")
    assert (v >= 64 and v & (v - 1) == 0) if have else v == -_lib.E_NO_DEVICE          # (an unknown key: -E_INVALID_ARG on any machine)
    assert lib.lz4flex_get_tuning(None, b"packed_scan_tiles") == -_lib.E_INVALID_ARG
    assert lib.lz4flex_set_tuning(None, b"packed_scan_tile", 512) == (-_lib.E_INVALID_ARG if have else -_lib.E_NO_DEVICE)   # read-only
