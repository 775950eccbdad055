"""CPU: lz4flex_decompress_batch_partial and lz4flex_decompress_partial_into -- the symbols, their bindings, the argument checks that need
no device, and the setting "decompress_partial"."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lz4flex_amd.h")
NAME = "lz4flex_decompress_batch_partial"
SCALAR = "lz4flex_decompress_partial_into"


def test_partial_entries_are_declared_exported_and_bound():
    from lz4_flex_amd import _lib, block, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", src)
    assert m, "not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["ctx", "in_base", "in_off", "in_len", "n", "out_base", "out_off", "target", "out_len",
                                                            "status", "mem_kind", "hip_stream"]
    m = re.search(r"\bint64_t\s+" + SCALAR + r"\s*\(([^;]*)\)\s*;", src)
    assert m, "not declared"
    assert [p.split()[-1].lstrip("*") for p in m.group(1).split(",")] == ["in", "in_len", "out", "target", "detail"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()]).decode()
    for name in (NAME, SCALAR):
        assert re.search(r" T " + name + r"\b", out), name
    V, U, I = C.c_void_p, C.c_uint32, C.c_int
    assert _lib.SIGNATURES[NAME] == (I, [V, V, V, V, U, V, V, V, V, V, I, V])
    res, args = _lib.SIGNATURES[SCALAR]
    assert res is C.c_int64 and args[:4] == [V, C.c_size_t, V, C.c_size_t] and len(args) == 5
    assert callable(block.decompress_partial) and callable(block.decompress_batch_partial) and callable(block.decompress_blocks_partial_device)
    # new symbols only: the number stays, callers detect them by the symbol
    assert _lib.load().lz4flex_abi_version() == 8
    note = open(HEADER).read().split("int lz4flex_abi_version")[0]
    assert NAME in note and SCALAR in note                 # (the version note names them)


def test_partial_argument_checks_and_no_cpu_path():
    """checks that need no device hold on any machine, before a context is looked at; a valid call without a device is -E_NO_DEVICE"""
    from lz4_flex_amd import _lib, block
    lib = _lib.load()
    src = np.frombuffer(b"\x50hello", np.uint8)
    io = np.zeros(1, np.uint64)
    il = np.array([len(src)], np.uint32)
    out = np.zeros(128, np.uint8)
    oo = np.zeros(1, np.uint64)
    tg = np.array([3], np.uint32)
    olen = np.zeros(1, np.uint32)
    st = np.zeros(1, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)     # noqa: E731
    NULL = C.c_void_p(0)

    def call(n=1, mem=_lib.MEM_HOST, **over):
        a = dict(in_off=p(io), in_len=p(il), out_off=p(oo), target=p(tg), out_len=p(olen), status=p(st))
        a.update(over)
        return getattr(lib, NAME)(None, p(src), a["in_off"], a["in_len"], n, p(out), a["out_off"], a["target"], a["out_len"], a["status"], mem, None)

    for name in ("in_off", "in_len", "out_off", "target", "out_len", "status"):
        assert call(**{name: NULL}) == -_lib.E_INVALID_ARG, name
    for mem in (7, 0x1001, _lib.MEM_DEVICE | _lib.MEM_CHAINED, _lib.MEM_HOST | _lib.MEM_CHAINED,
                _lib.MEM_DEVICE | _lib.MEM_BIG_BLOCKS | _lib.MEM_CHAINED):
        assert call(mem=mem) == -_lib.E_INVALID_ARG, hex(mem)
    assert call(n=0) == 0
    assert call(n=0, in_off=NULL, status=NULL, target=NULL) == 0
    assert call(n=0, mem=_lib.MEM_DEVICE | _lib.MEM_BIG_BLOCKS) == 0
    assert call(n=0, mem=7) == -_lib.E_INVALID_ARG           # (the memory kind is looked at before n)
    if lib.lz4flex_device_count() == 0:
        for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE, _lib.MEM_HOST | _lib.MEM_BIG_BLOCKS, _lib.MEM_DEVICE | _lib.MEM_BIG_BLOCKS):
            assert call(mem=mem) == -_lib.E_NO_DEVICE, hex(mem)
        assert getattr(lib, SCALAR)(p(src), len(src), p(out), 3, None) == -_lib.E_NO_DEVICE
        with pytest.raises(block.DeviceError):
            block.decompress_batch_partial(src, [0], [len(src)], out, [0], [3])
        with pytest.raises(block.DeviceError):
            block.decompress_partial(src.tobytes(), 3)
        assert olen[0] == 0 and st[0] == 0 and not out.any()
    # more than the u32 of the batch entry: refused before a context is looked at
    assert getattr(lib, SCALAR)(p(src), len(src), p(out), 1 << 32, None) == -_lib.E_INVALID_ARG


def test_decompress_partial_is_a_known_setting():
    """a known key answers with a context (or, without a device, with -E_NO_DEVICE: the default context); an unknown one is refused"""
    from lz4_flex_amd import _lib
    lib = _lib.load()
    assert lib.lz4flex_get_tuning(None, b"decompress_partial_") == -_lib.E_INVALID_ARG
    if lib.lz4flex_device_count() == 0:
        assert lib.lz4flex_get_tuning(None, b"decompress_partial") == -_lib.E_NO_DEVICE
        assert lib.lz4flex_set_tuning(None, b"decompress_partial", 0) == -_lib.E_NO_DEVICE
    else:
        ctx = C.c_void_p()
        assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
        try:
            assert lib.lz4flex_get_tuning(ctx, b"decompress_partial") == 1
            assert lib.lz4flex_set_tuning(ctx, b"decompress_partial", 0) == 0
            assert lib.lz4flex_get_tuning(ctx, b"decompress_partial") == 0
            assert lib.lz4flex_set_tuning(ctx, b"decompress_partial", 2) == -_lib.E_INVALID_ARG
        finally:
            lib.lz4flex_ctx_destroy(ctx)
    # the key is in the library and in the header's settings paragraph
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"decompress_partial\0" in blob
    assert open(HEADER).read().count('"decompress_partial"') >= 2
