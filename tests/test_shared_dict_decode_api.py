"""CPU: lz4flex_decompress_batch_shared_dict -- the symbol, its binding, the argument checks that need no device, and the setting
"decompress_shared_dict"."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lz4flex_amd.h")
NAME = "lz4flex_decompress_batch_shared_dict"


def test_shared_dict_decode_entry_is_declared_exported_and_bound():
    from lz4_flex_amd import _lib, block, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", src)
    assert m, "not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 15
    # ctx, in_base, in_off, in_len, n, out_base, out_off, out_cap, out_len, status, detail, dict, dict_len, mem_kind, hip_stream
    assert [p.split()[-1].lstrip("*") for p in params] == ["ctx", "in_base", "in_off", "in_len", "n", "out_base", "out_off", "out_cap", "out_len",
                                                            "status", "detail", "dict", "dict_len", "mem_kind", "hip_stream"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()]).decode()
    assert re.search(r" T " + NAME + r"\b", out)
    res, args = _lib.SIGNATURES[NAME]
    V, U, I = C.c_void_p, C.c_uint32, C.c_int
    assert res is I and args == [V, V, V, V, U, V, V, V, V, V, V, V, U, I, V]
    assert callable(block.decompress_batch_with_shared_dict) and callable(block.decompress_blocks_with_shared_dict_device)
    # the entry changes nothing for an existing call: the number stays, callers detect it by the symbol
    assert _lib.load().lz4flex_abi_version() == 8
    assert NAME in open(HEADER).read().split("int lz4flex_abi_version")[0]        # (the version note names it)


def test_shared_dict_decode_argument_checks_and_no_cpu_path():
    """checks that need no device hold on any machine; a valid call without a device is -E_NO_DEVICE (no CPU path)"""
    from lz4_flex_amd import _lib, block
    lib = _lib.load()
    src = np.frombuffer(b"\x50hello", np.uint8)
    dic = np.frombuffer(b"hello dictionary", np.uint8)
    io = np.zeros(1, np.uint64)
    il = np.array([len(src)], np.uint32)
    out = np.zeros(128, np.uint8)
    oo = np.zeros(1, np.uint64)
    oc = np.array([128], np.uint32)
    olen = np.zeros(1, np.uint32)
    st = np.zeros(1, np.int32)
    det = np.zeros(2, np.uint64)
    p = lambda a: C.c_void_p(a.ctypes.data)     # noqa: E731
    NULL = C.c_void_p(0)

    def call(n=1, mem=_lib.MEM_HOST, d=p(dic), dlen=len(dic), detail=p(det), **over):
        a = dict(in_off=p(io), in_len=p(il), out_off=p(oo), out_cap=p(oc), out_len=p(olen), status=p(st))
        a.update(over)
        return getattr(lib, NAME)(None, p(src), a["in_off"], a["in_len"], n, p(out), a["out_off"], a["out_cap"], a["out_len"], a["status"],
                                  detail, d, dlen, mem, None)

    for name in ("in_off", "in_len", "out_off", "out_cap", "out_len", "status"):
        assert call(**{name: NULL}) == -_lib.E_INVALID_ARG, name
    assert call(d=NULL, dlen=5) == -_lib.E_INVALID_ARG                       # a length without a dictionary
    assert call(mem=7) == -_lib.E_INVALID_ARG
    assert call(mem=_lib.MEM_DEVICE | _lib.MEM_CHAINED) == -_lib.E_INVALID_ARG
    assert call(mem=_lib.MEM_HOST | _lib.MEM_CHAINED) == -_lib.E_INVALID_ARG
    assert call(mem=_lib.MEM_DEVICE | _lib.MEM_BIG_BLOCKS | _lib.MEM_CHAINED) == -_lib.E_INVALID_ARG
    assert call(n=0) == 0
    assert call(n=0, in_off=NULL, status=NULL, detail=NULL) == 0
    assert call(n=0, mem=_lib.MEM_DEVICE | _lib.MEM_BIG_BLOCKS) == 0
    if lib.lz4flex_device_count() == 0:
        assert call() == -_lib.E_NO_DEVICE
        assert call(detail=NULL) == -_lib.E_NO_DEVICE
        assert call(d=NULL, dlen=0) == -_lib.E_NO_DEVICE                      # (lz4flex_decompress_batch)
        assert call(mem=_lib.MEM_DEVICE) == -_lib.E_NO_DEVICE
        assert call(mem=_lib.MEM_HOST | _lib.MEM_BIG_BLOCKS) == -_lib.E_NO_DEVICE
        with pytest.raises(block.DeviceError):
            block.decompress_batch_with_shared_dict(src, [0], [len(src)], dic, out, [0], [128])
        assert olen[0] == 0 and st[0] == 0 and not out.any()


def test_decompress_shared_dict_is_a_known_setting():
    """a known key answers with a context (or, without a device, with -E_NO_DEVICE: the default context); an unknown one is refused"""
    from lz4_flex_amd import _lib
    lib = _lib.load()
    if lib.lz4flex_device_count() == 0:
        assert lib.lz4flex_get_tuning(None, b"decompress_shared_dict") == -_lib.E_NO_DEVICE
        assert lib.lz4flex_set_tuning(None, b"decompress_shared_dict", 0) == -_lib.E_NO_DEVICE
    else:
        ctx = C.c_void_p()
        assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
        try:
            assert lib.lz4flex_get_tuning(ctx, b"decompress_shared_dict") == 1
            assert lib.lz4flex_set_tuning(ctx, b"decompress_shared_dict", 0) == 0
            assert lib.lz4flex_get_tuning(ctx, b"decompress_shared_dict") == 0
            assert lib.lz4flex_set_tuning(ctx, b"decompress_shared_dict", 2) == -_lib.E_INVALID_ARG
            assert lib.lz4flex_get_tuning(ctx, b"decompress_shared_dikt") == -_lib.E_INVALID_ARG
        finally:
            lib.lz4flex_ctx_destroy(ctx)
    # the key is in the library and in the header's settings paragraph
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"decompress_shared_dict\0" in blob
    assert '"decompress_shared_dict"' in open(HEADER).read()
