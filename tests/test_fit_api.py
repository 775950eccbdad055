"""CPU test of the fit entries (lz4flex_fit_batch, lz4flex_compress_fit_work_size, lz4flex_compress_batch_fit): declared, exported and
bound; every argument check answers before a context or a device is looked at; valid calls fail loudly without a device; the header
states the rule the model implements.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lz4flex_amd.h")
ENTRIES = ["lz4flex_fit_batch", "lz4flex_compress_fit_work_size", "lz4flex_compress_batch_fit"]


@pytest.fixture(scope="module")
def lib():
    from lz4_flex_amd import _lib, build
    build.build()
    return _lib.load()


def test_declared_exported_and_bound(lib):
    from lz4_flex_amd import _lib, block, build
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(lz4flex_[a-z0-9_]+)\s*\(", src))
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB]).decode()
    exported = set(re.findall(r" T (lz4flex_[a-z0-9_]+)", out))
    note = text[text.index("The round of this header:"):text.index("int lz4flex_abi_version(void);")]
    for name in ENTRIES:
        assert name in declared and name in exported and name in _lib.SIGNATURES, name
    assert "lz4flex_fit_batch" in note and "lz4flex_compress_batch_fit" in note and '"fit_serial"' in note
    assert len(_lib.SIGNATURES["lz4flex_fit_batch"][1]) == 16 and len(_lib.SIGNATURES["lz4flex_compress_batch_fit"][1]) == 16
    for name in ("fit_batch", "compress_batch_fit", "fit_blocks_device", "compress_blocks_fit_device", "compress_fit"):
        assert callable(getattr(block, name)), name
    assert b"lz4_fit_kernel" in open(build.LIB, "rb").read() and b"lz4_fit_serial_kernel" in open(build.LIB, "rb").read()
    # the work size is the packed entries' (their scan is reused), with or without a device
    for n in (0, 1, 1024, 1025, 100000):
        assert lib.lz4flex_compress_fit_work_size(n) == lib.lz4flex_packed_work_size(n)


def test_the_header_states_the_rule_of_the_model(lib):
    text = open(HEADER).read()
    for line in ("`ext(x) = 0 if x < 15 else 1 + (x-15)/255`", "`tail(L) = 1 + ext(L) + L`", "`len(B) <= cap`", "`c_k < cap`",
                 "`L = Lfit(cap - c_k, n - p_k)`", "`max(5, 12 - m_{k-1})`", "`m_k >= 5`", "`h = 1 + ext(l_k) + l_k + 2`", "`b = cap - c_k - h - 1`",
                 "`b >= 5`", "`m' = min(m_k - 1, 18 + 255*(b - 5))`", "`max(5, 12 - m') <= b`", "`L = Lfit(cap - c_k - h - ext(m'-4), n - p_k - l_k - m')`",
                 "`L >= max(5, 12 - m')`", "`used = p_k + l_k + m' + L`", "the largest `used`; ties go to the smallest size, then the smallest `k`, then Plain before Clipped",
                 "only at `cap == 0`", '"fit_serial"', "SELF-CONTAINED blocks only", "The arguments are checked before a context or a device is looked at"):
        assert line in text, line


def _args():
    """a valid 1-block batch as ctypes arrays (host memory; a device pointer is never followed by an argument check)"""
    return dict(blk=C.create_string_buffer(bytes([0x50]) + b"hello", 16), blk_off=(C.c_uint64 * 1)(0), blk_len=(C.c_uint32 * 1)(6),
                src=C.create_string_buffer(b"hello", 16), src_off=(C.c_uint64 * 1)(0), src_len=(C.c_uint32 * 1)(5),
                out=C.create_string_buffer(b"\xC5" * 64, 64), out_off=(C.c_uint64 * 1)(0), out_cap=(C.c_uint32 * 1)(4),
                out_len=(C.c_uint32 * 1)(7), in_used=(C.c_uint32 * 1)(7), status=(C.c_int32 * 1)(7), scratch=C.create_string_buffer(64),
                work=C.create_string_buffer(4096))


def _fit(lib, a, n=1, mem=0, **over):
    a = dict(a, **over)
    return lib.lz4flex_fit_batch(None, a["blk"], a["blk_off"], a["blk_len"], a["src"], a["src_off"], a["src_len"], n, a["out"], a["out_off"],
                                 a["out_cap"], a["out_len"], a["in_used"], a["status"], mem, None)


def _compress(lib, a, n=1, mem=0, **over):
    a = dict(a, **over)
    return lib.lz4flex_compress_batch_fit(None, a["src"], a["src_off"], a["src_len"], n, a["scratch"], 64, a["out"], a["out_off"], a["out_cap"],
                                          a["out_len"], a["in_used"], a["status"], a["work"], mem, None)


CALLS = [("fit", _fit, ("blk_off", "blk_len", "src_off", "src_len", "out_off", "out_cap", "out_len", "in_used", "status")),
         ("compress_fit", _compress, ("src_off", "src_len", "out_off", "out_cap", "out_len", "in_used", "status"))]


def test_argument_checks_need_no_device(lib):
    from lz4_flex_amd import _lib
    INV = -_lib.E_INVALID_ARG
    a = _args()
    HOST, DEV, BIG, CHAINED = _lib.MEM_HOST, _lib.MEM_DEVICE, _lib.MEM_BIG_BLOCKS, _lib.MEM_CHAINED
    for what, call, arrays in CALLS:
        for mem in (HOST, DEV, HOST | BIG, DEV | BIG):
            for name in arrays:
                assert call(lib, a, mem=mem, **{name: None}) == INV, (what, name)
        for mem in (7, HOST | CHAINED, DEV | CHAINED, DEV | CHAINED | BIG, 0x1001):
            assert call(lib, a, mem=mem) == INV, (what, hex(mem))
        assert call(lib, a, n=0, mem=9) == INV, what                      # a bad mem_kind is refused even when there is nothing to do
    # scratch and work: a DEVICE call needs them, a HOST call does not look at them
    assert _compress(lib, a, mem=DEV, scratch=None) == INV and _compress(lib, a, mem=DEV | BIG, work=None) == INV
    assert (a["out_len"][0], a["in_used"][0], a["status"][0], a["out"].raw) == (7, 7, 7, b"\xC5" * 64)     # nothing of the results was touched


def test_nothing_to_do_and_no_device(lib):
    from lz4_flex_amd import _lib, block
    a = _args()
    HOST, DEV, BIG = _lib.MEM_HOST, _lib.MEM_DEVICE, _lib.MEM_BIG_BLOCKS
    for what, call, arrays in CALLS:
        for mem in (HOST, DEV, HOST | BIG, DEV | BIG):
            assert call(lib, a, n=0, mem=mem) == 0, (what, mem)
            assert call(lib, a, n=0, mem=mem, scratch=None, work=None, **{k: None for k in arrays}) == 0, what
    if lib.lz4flex_device_count() == 0:
        NODEV = -_lib.E_NO_DEVICE
        for what, call, _arrays in CALLS:
            assert call(lib, a) == NODEV and call(lib, a, mem=HOST | BIG) == NODEV, what
        assert _compress(lib, a, scratch=None, work=None) == NODEV
        assert (a["out_len"][0], a["in_used"][0], a["status"][0], a["out"].raw) == (7, 7, 7, b"\xC5" * 64)
        x, out = np.frombuffer(b"hello, hello, hello", np.uint8), np.zeros(64, np.uint8)
        with pytest.raises(block.DeviceError):
            block.fit_batch(np.frombuffer(bytes([0x50]) + b"hello", np.uint8), [0], [6], x, [0], [5], out, [0], [4])
        with pytest.raises(block.DeviceError):
            block.compress_batch_fit(x, [0], [x.size], out, [0], [12])
        with pytest.raises(block.DeviceError):
            block.compress_fit(b"hello, hello, hello", 12)


def test_fit_serial_is_a_known_key(lib):
    from lz4_flex_amd import _lib
    have = lib.lz4flex_device_count() > 0
    assert lib.lz4flex_get_tuning(None, b"fit_serial") == (0 if have else -_lib.E_NO_DEVICE)      # (an unknown key: -E_INVALID_ARG on any machine)
    assert lib.lz4flex_get_tuning(None, b"fit_serial_") == -_lib.E_INVALID_ARG
    assert lib.lz4flex_set_tuning(None, b"fit_serial", 2) == (-_lib.E_INVALID_ARG if have else -_lib.E_NO_DEVICE)


def test_python_wrappers_refuse_arrays_of_different_lengths(lib):
    import torch
    from lz4_flex_amd import block
    x, out = np.zeros(32, np.uint8), np.zeros(64, np.uint8)
    with pytest.raises(ValueError):
        block.fit_batch(x, [0, 8], [8], x, [0, 8], [8, 8], out, [0, 32], [32, 32])
    with pytest.raises(ValueError):
        block.fit_batch(x, [0, 8], [8, 8], x, [0], [8], out, [0, 32], [32, 32])
    with pytest.raises(ValueError):
        block.compress_batch_fit(x, [0, 8], [8, 8], out, [0, 32], [32])
    host, z = torch.zeros(64, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError):
        block.fit_blocks_device(host, z, z, host, z, z, z)
    with pytest.raises(ValueError):
        block.compress_blocks_fit_device(host, z, z, z)
