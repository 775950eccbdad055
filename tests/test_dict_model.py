"""CPU: the geometry of dictionary items on the throughput encoder (lz4flex_compress_batch_ex, compress_mode fast), pinned on the scalar
model before any GPU runs it, and the C ABI of the new entry point."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dict_cases as D
import oracle_api as O
import wave_model as W


@pytest.mark.parametrize("kind", D.KINDS)
def test_model_item_decodes_with_tail_and_with_whole_dictionary(kind):
    """lz4w_compress(dict[-h:] + block, hist = h) for every h and block length: the oracle's decompress_into_with_dict returns the
    block with the dictionary's tail and with the whole 1 MiB dictionary (matches reach only into its last h bytes)"""
    d = D.dictionary(kind)
    for n in D.LENS:
        b = D.block(kind, n)
        for h in D.HS:
            c = D.model(b, d[-h:])
            assert D.model(b, d) == c if h == W.HIST else True
            assert D.oracle_decodes(c, b, d[-h:]), (n, h)
            assert D.oracle_decodes(c, b, d), (n, h)


def test_full_history_is_the_linked_history_path():
    """h == HIST: a dictionary item is exactly what LZ4FLEX_BLOCK_HISTORY(32768) encodes -- the model's history path over the same
    96 KiB (32 KiB of dictionary tail, a 64 KiB block)"""
    for kind in ("json", "text", "log"):
        d = D.dictionary(kind)
        b = D.block(kind, 65536)
        assert D.model(b, d) == W.compress(d[-W.HIST:] + b, hist=W.HIST)


def test_dictionary_shrinks_small_log_records():
    """64 records of 4 KiB from the log stream: against a 1 MiB dictionary of other log lines (its last 32 KiB count) the model writes
    0.273 of the input, without one 0.391 (measured on the model; the bar is set at 0.85 x)"""
    d = D.dictionary("log")
    with_d = without = 0
    for i in range(64):
        b = D.block("log", 4096, salt=i)
        c = D.model(b, d)
        assert D.oracle_decodes(c, b, d)
        with_d += len(c)
        without += len(W.compress(b, sub=1))
    assert with_d < 0.85 * without, (with_d, without)


def test_empty_block_is_one_token():
    for h in (1, 4096, W.HIST):
        assert D.model(b"", D.dictionary("json")[-h:]) == b"\0"


HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lz4flex_amd.h")


def test_compress_batch_ex_is_declared_exported_and_bound():
    from lz4_flex_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\blz4flex_compress_batch_ex\s*\(", src)
    assert re.search(r"typedef struct lz4flex_compress_ext\s*\{", src)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()]).decode()
    assert re.search(r" T lz4flex_compress_batch_ex\b", out)
    assert "lz4flex_compress_batch_ex" in _lib.SIGNATURES
    assert [f[0] for f in _lib.CompressExt._fields_] == ["dict_base", "dict_off", "dict_len"]
    assert C.sizeof(_lib.CompressExt) == 24
    assert _lib.load().lz4flex_abi_version() == 8


def test_compress_batch_ex_argument_checks_and_no_cpu_path():
    """checks that need no device hold on any machine; a valid call without a device is -E_NO_DEVICE (no CPU path)"""
    from lz4_flex_amd import _lib, block
    lib = _lib.load()
    src = np.frombuffer(b"hello hello hello hello", np.uint8)
    dic = np.frombuffer(b"hello dictionary", np.uint8)
    io = np.zeros(1, np.uint64)
    il = np.array([len(src)], np.uint32)
    do = np.zeros(1, np.uint64)
    dl = np.array([len(dic)], np.uint32)
    out = np.zeros(128, np.uint8)
    oo = np.zeros(1, np.uint64)
    oc = np.array([128], np.uint32)
    olen = np.zeros(1, np.uint32)
    st = np.zeros(1, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)     # noqa: E731

    def call(ext, mem=_lib.MEM_HOST, in_off=None):
        return lib.lz4flex_compress_batch_ex(None, p(src), in_off if in_off is not None else p(io), p(il), None, 1, p(out), p(oo), p(oc),
                                             p(olen), p(st), C.byref(ext) if ext is not None else None, mem, None)

    E = _lib.CompressExt
    assert call(E(dic.ctypes.data, None, dl.ctypes.data)) == -_lib.E_INVALID_ARG            # dict_base without dict_off
    assert call(E(dic.ctypes.data, do.ctypes.data, None)) == -_lib.E_INVALID_ARG            # ... without dict_len
    assert call(E(dic.ctypes.data, do.ctypes.data, dl.ctypes.data), in_off=C.c_void_p(0)) == -_lib.E_INVALID_ARG
    assert call(E(dic.ctypes.data, do.ctypes.data, dl.ctypes.data), mem=7) == -_lib.E_INVALID_ARG
    assert call(E(dic.ctypes.data, do.ctypes.data, dl.ctypes.data), mem=_lib.MEM_DEVICE | _lib.MEM_CHAINED) == -_lib.E_INVALID_ARG
    if lib.lz4flex_device_count() == 0:
        assert call(E(dic.ctypes.data, do.ctypes.data, dl.ctypes.data)) == -_lib.E_NO_DEVICE
        assert call(None) == -_lib.E_NO_DEVICE
        with pytest.raises(block.DeviceError):
            block.compress_batch_with_dict(src, [0], [len(src)], dic, [0], [len(dic)], out, [0], [128])
        with pytest.raises(block.DeviceError):
            block.decompress_batch_with_dict(src, [0], [len(src)], dic, [0], [len(dic)], out, [0], [128])
        assert olen[0] == 0 and st[0] == 0 and not out.any()
