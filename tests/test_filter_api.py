"""CPU test of the typed batch entries (lz4flex_filter_batch, lz4flex_compress_batch_typed, lz4flex_decompress_batch_typed): declared,
exported and bound; the ABI number stays; every argument check answers before a context or a device is looked at; valid calls fail
loudly without a device; the Python wrappers refuse what they cannot pass on.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lz4flex_amd.h")
ENTRIES = ["lz4flex_filter_batch", "lz4flex_compress_batch_typed", "lz4flex_decompress_batch_typed"]


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
    note = text[text.index("The round of this header: 8"):text.index("int lz4flex_abi_version(void);")]
    for name in ENTRIES:
        assert name in declared and name in exported and name in _lib.SIGNATURES and name in note, name
    for name, value in (("LZ4FLEX_FILTER_NONE", 0), ("LZ4FLEX_FILTER_SHUFFLE", 1), ("LZ4FLEX_FILTER_BITSHUFFLE", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), src), name
    assert (_lib.FILTER_NONE, _lib.FILTER_SHUFFLE, _lib.FILTER_BITSHUFFLE) == (0, 1, 2)
    assert block.FILTERS == {"none": 0, "shuffle": 1, "bitshuffle": 2}
    assert lib.lz4flex_abi_version() == 8
    # the header carries the definition
    for line in ("`out[j*m + e] = in[e*E + j]`", "`m8 = (L / E) / 8 * 8`", "Bit `b` (LSB = 0) of byte `q` of plane `p` is bit `k` of `in[(8q + b)*E + j]`",
                 '"filter_bytewise"'):
        assert line in text, line


def _args():
    """a valid 1-block batch as ctypes arrays (host memory; a device pointer is never followed by an argument check)"""
    return dict(src=C.create_string_buffer(bytes(range(16)), 16), in_off=(C.c_uint64 * 1)(0), in_len=(C.c_uint32 * 1)(16),
                out=C.create_string_buffer(b"\xC5" * 64, 64), out_off=(C.c_uint64 * 1)(0), out_cap=(C.c_uint32 * 1)(64),
                out_len=(C.c_uint32 * 1)(7), status=(C.c_int32 * 1)(7), detail=(C.c_uint64 * 2)(7, 7), tmp=C.create_string_buffer(64),
                tmp_off=(C.c_uint64 * 1)(0))


def _filter(lib, a, n=1, filt=1, elem=2, inverse=0, mem=0, **over):
    a = dict(a, **over)
    return lib.lz4flex_filter_batch(None, a["src"], a["in_off"], a["in_len"], n, a["out"], a["out_off"], filt, elem, inverse, mem, None)


def _compress(lib, a, n=1, filt=1, elem=2, mem=0, **over):
    a = dict(a, **over)
    return lib.lz4flex_compress_batch_typed(None, a["src"], a["in_off"], a["in_len"], n, a["out"], a["out_off"], a["out_cap"], a["out_len"],
                                            a["status"], filt, elem, a["tmp"], a["tmp_off"], mem, None)


def _decompress(lib, a, n=1, filt=1, elem=2, mem=0, **over):
    a = dict(a, **over)
    return lib.lz4flex_decompress_batch_typed(None, a["src"], a["in_off"], a["in_len"], n, a["out"], a["out_off"], a["out_cap"], a["out_len"],
                                              a["status"], a["detail"], filt, elem, a["tmp"], a["tmp_off"], mem, None)


CALLS = [("filter", _filter, ("in_off", "in_len", "out_off")),
         ("compress", _compress, ("in_off", "in_len", "out_off", "out_cap", "out_len", "status")),
         ("decompress", _decompress, ("in_off", "in_len", "out_off", "out_cap", "out_len", "status"))]


def test_argument_checks_need_no_device(lib):
    from lz4_flex_amd import _lib
    INV = -_lib.E_INVALID_ARG
    a = _args()
    HOST, DEV, BIG, CHAINED = _lib.MEM_HOST, _lib.MEM_DEVICE, _lib.MEM_BIG_BLOCKS, _lib.MEM_CHAINED
    for what, call, arrays in CALLS:
        for mem in (HOST, DEV, HOST | BIG, DEV | BIG):
            for filt in (-1, 3, 99):
                assert call(lib, a, filt=filt, mem=mem) == INV, (what, filt)
            for elem in (0, 3, 5, 6, 7, 16, 0x80000000):
                assert call(lib, a, elem=elem, mem=mem) == INV, (what, elem)
                assert call(lib, a, filt=0, elem=elem, mem=mem) == INV, (what, elem)
            for name in arrays:
                assert call(lib, a, mem=mem, **{name: None}) == INV, (what, name)
                assert call(lib, a, filt=0, mem=mem, **{name: None}) == INV, (what, name)
        for mem in (7, HOST | CHAINED, DEV | CHAINED, DEV | CHAINED | BIG, 0x1001):
            assert call(lib, a, mem=mem) == INV, (what, hex(mem))
        # the bad scalar arguments are refused even when there is nothing to do
        assert call(lib, a, n=0, filt=3) == INV and call(lib, a, n=0, elem=3) == INV and call(lib, a, n=0, mem=9) == INV, what
    # the tmp slots: a DEVICE call with a filter needs them, a HOST call and FILTER_NONE do not look at them
    for call in (_compress, _decompress):
        for filt in (1, 2):
            assert call(lib, a, filt=filt, mem=DEV, tmp=None) == INV and call(lib, a, filt=filt, mem=DEV | BIG, tmp_off=None) == INV
    # nothing of the results was touched
    assert (a["out_len"][0], a["status"][0], a["detail"][0], a["out"].raw) == (7, 7, 7, b"\xC5" * 64)


def test_nothing_to_do_and_no_device(lib):
    from lz4_flex_amd import _lib, block
    a = _args()
    HOST, DEV, BIG = _lib.MEM_HOST, _lib.MEM_DEVICE, _lib.MEM_BIG_BLOCKS
    for what, call, arrays in CALLS:
        for mem in (HOST, DEV, HOST | BIG, DEV | BIG):
            for filt in (0, 1, 2):
                for elem in (1, 2, 4, 8):
                    assert call(lib, a, n=0, filt=filt, elem=elem, mem=mem) == 0, (what, filt, elem, mem)
            assert call(lib, a, n=0, mem=mem, tmp=None, tmp_off=None, **{k: None for k in arrays}) == 0, what
    if lib.lz4flex_device_count() == 0:
        NODEV = -_lib.E_NO_DEVICE
        for what, call, _arrays in CALLS:
            for filt in (0, 1, 2):
                for elem in (1, 2, 4, 8):
                    assert call(lib, a, filt=filt, elem=elem) == NODEV, (what, filt, elem)
            assert call(lib, a, mem=HOST | BIG) == NODEV and call(lib, a, mem=HOST, tmp=None, tmp_off=None) == NODEV, what
        assert _filter(lib, a, inverse=1) == NODEV
        assert (a["out_len"][0], a["status"][0], a["out"].raw) == (7, 7, b"\xC5" * 64)
        x, out = np.arange(16, dtype=np.uint8), np.zeros(64, np.uint8)
        with pytest.raises(block.DeviceError):
            block.filter_batch(x, [0], [16], out, [0], "shuffle", 2)
        with pytest.raises(block.DeviceError):
            block.compress_batch_typed(x, [0], [16], out, [0], [64], "bitshuffle", 4)
        with pytest.raises(block.DeviceError):
            block.decompress_batch_typed(x, [0], [16], out, [0], [64], 2, 8)


def test_filter_bytewise_is_a_known_key(lib):
    from lz4_flex_amd import _lib
    have = lib.lz4flex_device_count() > 0
    assert lib.lz4flex_get_tuning(None, b"filter_bytewise") == (0 if have else -_lib.E_NO_DEVICE)      # (an unknown key: -E_INVALID_ARG on any machine)
    assert lib.lz4flex_get_tuning(None, b"filter_bytewise_") == -_lib.E_INVALID_ARG
    assert lib.lz4flex_set_tuning(None, b"filter_bytewise", 2) == (-_lib.E_INVALID_ARG if have else -_lib.E_NO_DEVICE)


def test_python_wrappers_refuse_bad_arguments(lib):
    import torch
    from lz4_flex_amd import block
    x, out = np.arange(16, dtype=np.uint8), np.zeros(64, np.uint8)
    for filt in ("", "Shuffle", "bit", 3, -1, None, 1.0, True):
        with pytest.raises(ValueError):
            block.filter_batch(x, [0], [16], out, [0], filt, 2)
        with pytest.raises(ValueError):
            block.compress_batch_typed(x, [0], [16], out, [0], [64], filt, 2)
        with pytest.raises(ValueError):
            block.decompress_batch_typed(x, [0], [16], out, [0], [64], filt, 2)
    for elem in (0, 3, 16, "2", 2.0, None, True):
        with pytest.raises(ValueError):
            block.filter_batch(x, [0], [16], out, [0], "shuffle", elem)
        with pytest.raises(ValueError):
            block.compress_batch_typed(x, [0], [16], out, [0], [64], 1, elem)
        with pytest.raises(ValueError):
            block.decompress_batch_typed(x, [0], [16], out, [0], [64], 2, elem)
    with pytest.raises(ValueError):
        block.filter_batch(x, [0, 8], [8], out, [0, 8], "shuffle", 2)
    with pytest.raises(ValueError):
        block.filter_batch(x, [0, 8], [8, 8], out, [0], "shuffle", 2)
    with pytest.raises(ValueError):
        block.compress_batch_typed(x, [0, 8], [8, 8], out, [0, 32], [32], "shuffle", 2)
    with pytest.raises(ValueError):
        block.decompress_batch_typed(x, [0], [8, 8], out, [0], [32], "shuffle", 2)
    # the tensor forms take contiguous tensors on the GPU, of dtypes of 1, 2, 4 or 8 bytes, in blocks the element size divides
    host = torch.zeros(64, dtype=torch.float32)
    with pytest.raises(ValueError):
        block.compress_tensor(host)
    with pytest.raises(ValueError):
        block.compress_tensor(np.zeros(64, np.float32))
    with pytest.raises(ValueError):
        block.compress_tensor(host, filter="lz")
    with pytest.raises(ValueError):
        block.filter_blocks_device(host.view(torch.uint8), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), "shuffle", 4)
    with pytest.raises(ValueError):
        block.compress_blocks_typed_device(host.view(torch.uint8), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), "shuffle", 3)
    with pytest.raises(ValueError):
        block.decompress_blocks_typed_device(host.view(torch.uint8), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64),
                                             torch.zeros(1, dtype=torch.int64), "shuffle", 4)
