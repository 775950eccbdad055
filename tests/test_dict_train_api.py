"""CPU test of the dictionary trainer's entry points (lz4flex_dict_train, lz4flex_dict_train_work_size): declared, exported and bound; the
ABI number stays and the header's version note names the entry; every argument check answers before a context or a device is looked at;
an empty HOST call needs no device; the workspace grows with the batch.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lz4flex_amd.h")
ENTRIES = ["lz4flex_dict_train", "lz4flex_dict_train_work_size"]


@pytest.fixture(scope="module")
def lib():
    from lz4_flex_amd import _lib, build
    build.build()
    return _lib.load()


def test_declared_exported_and_bound(lib):
    from lz4_flex_amd import _lib, build
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(lz4flex_[a-z0-9_]+)\s*\(", src))
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB]).decode()
    exported = set(re.findall(r" T (lz4flex_[a-z0-9_]+)", out))
    for name in ENTRIES:
        assert name in declared and name in exported and name in _lib.SIGNATURES, name
    assert lib.lz4flex_abi_version() == 8
    note = text[text.index("The round of this header: 8"):text.index("int lz4flex_abi_version(void);")]
    assert "lz4flex_dict_train" in note and "lz4flex_dict_train_work_size" in note


def _args():
    """a valid 2-sample batch as ctypes arrays (host memory; a device pointer is never followed by an argument check)"""
    return dict(src=C.create_string_buffer(b"0123456789abcdef" * 4, 64), in_off=(C.c_uint64 * 2)(0, 32), in_len=(C.c_uint32 * 2)(32, 32),
                out=C.create_string_buffer(65536), dict_len=(C.c_uint32 * 1)(7), status=(C.c_int32 * 1)(7), work=C.create_string_buffer(64))


def _train(lib, a, n=2, cap=1024, segment=512, mem=0, **over):
    a = dict(a, **over)
    return lib.lz4flex_dict_train(None, a["src"], a["in_off"], a["in_len"], n, a["out"], cap, segment, a["dict_len"], a["status"], a["work"],
                                  mem, None)


def test_argument_checks_need_no_device(lib):
    from lz4_flex_amd import _lib
    INV = -_lib.E_INVALID_ARG
    a = _args()
    HOST, DEV = _lib.MEM_HOST, _lib.MEM_DEVICE
    for mem in (HOST, DEV, HOST | _lib.MEM_BIG_BLOCKS, DEV | _lib.MEM_BIG_BLOCKS):
        for segment in (1, 63, 2049, 4096, 0xFFFFFFFF):
            assert _train(lib, a, segment=segment, mem=mem) == INV, segment
        for cap in (65537, 1 << 20, 0xFFFFFFFF):
            assert _train(lib, a, cap=cap, mem=mem) == INV, cap
        for name in ("in_off", "in_len", "dict_len", "status", "out"):
            assert _train(lib, a, mem=mem, **{name: None}) == INV, name
        # the bad arguments are refused even when there is nothing to do
        assert _train(lib, a, n=0, segment=63, mem=mem) == INV and _train(lib, a, n=0, cap=65537, mem=mem) == INV
        assert _train(lib, a, n=0, mem=mem, dict_len=None) == INV and _train(lib, a, cap=0, mem=mem, status=None) == INV
    assert _train(lib, a, mem=DEV, work=None) == INV and _train(lib, a, n=0, mem=DEV, work=None) == INV
    for mem in (7, HOST | _lib.MEM_CHAINED, DEV | _lib.MEM_CHAINED, DEV | _lib.MEM_CHAINED | _lib.MEM_BIG_BLOCKS, 0x1001):
        assert _train(lib, a, mem=mem) == INV, hex(mem)
        assert _train(lib, a, n=0, mem=mem) == INV, hex(mem)
    assert (a["dict_len"][0], a["status"][0]) == (7, 7)            # nothing of the results was touched


def test_nothing_to_do_and_no_device(lib):
    from lz4_flex_amd import _lib, block
    for mem in (_lib.MEM_HOST, _lib.MEM_HOST | _lib.MEM_BIG_BLOCKS):
        for segment in (0, 64, 512, 2048):
            a = _args()
            assert _train(lib, a, n=0, segment=segment, mem=mem) == 0 and (a["dict_len"][0], a["status"][0]) == (0, 0)
            a = _args()
            assert _train(lib, a, n=0, segment=segment, mem=mem, src=None, in_off=None, in_len=None, work=None) == 0
            assert (a["dict_len"][0], a["status"][0]) == (0, 0)
            a = _args()
            assert _train(lib, a, cap=0, segment=segment, mem=mem, out=None, work=None) == 0 and (a["dict_len"][0], a["status"][0]) == (0, 0)
    assert block.train_dictionary([]) == b"" and block.train_dictionary([b"some sample"], dict_size=0) == b""
    if lib.lz4flex_device_count() == 0:
        NODEV = -_lib.E_NO_DEVICE
        a = _args()
        for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE, _lib.MEM_DEVICE | _lib.MEM_BIG_BLOCKS):
            for segment in (0, 64, 2048):
                assert _train(lib, a, segment=segment, mem=mem) == NODEV
        assert _train(lib, a, n=0, mem=_lib.MEM_DEVICE) == NODEV and _train(lib, a, cap=0, mem=_lib.MEM_DEVICE) == NODEV
        assert (a["dict_len"][0], a["status"][0]) == (7, 7)
        with pytest.raises(block.DeviceError):
            block.train_dictionary([b"no gpu, no trainer"] * 3)
        with pytest.raises(block.DeviceError):
            block.train_dictionary_batch(np.frombuffer(b"no gpu, no trainer", np.uint8), [0, 4], [18, 14], dict_size=100, segment=64)


def test_work_size_grows_with_the_batch(lib):
    sizes = [int(lib.lz4flex_dict_train_work_size(n)) for n in (0, 1, 2, 1024, 1025, 65536, 1 << 20, 0xFFFFFFFF)]
    assert sizes == sorted(sizes) and sizes[0] >= 4 << 20
    assert sizes[5] - sizes[0] >= 16 * 65536                       # two words of 8 bytes per sample
    assert sizes[5] <= (4 << 20) + 65536 + 17 * 65536 + 8192      # ... the counters, the staging area and little else
    assert sizes[-1] > 16 * 0xFFFFFFFF                             # no 32-bit arithmetic on the way
