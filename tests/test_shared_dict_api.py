"""CPU: lz4flex_compress_batch_shared_dict -- the symbol, its binding, the argument checks that need no device, and the digest's
geometry (hs) as the header states it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lz4flex_amd.h")


def test_shared_dict_entry_is_declared_exported_and_bound():
    from lz4_flex_amd import _lib, block, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\blz4flex_compress_batch_shared_dict\s*\(", src)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()]).decode()
    assert re.search(r" T lz4flex_compress_batch_shared_dict\b", out)
    assert "lz4flex_compress_batch_shared_dict" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["lz4flex_compress_batch_shared_dict"][1]) == 14
    assert callable(block.compress_batch_with_shared_dict) and callable(block.compress_blocks_with_shared_dict_device)
    # the entry changes nothing for an existing call: the number stays, callers detect it by the symbol
    assert _lib.load().lz4flex_abi_version() == 8


def test_shared_dict_argument_checks_and_no_cpu_path():
    """checks that need no device hold on any machine; a valid call without a device is -E_NO_DEVICE (no CPU path)"""
    from lz4_flex_amd import _lib, block
    lib = _lib.load()
    src = np.frombuffer(b"hello hello hello hello", np.uint8)
    dic = np.frombuffer(b"hello dictionary", np.uint8)
    io = np.zeros(1, np.uint64)
    il = np.array([len(src)], np.uint32)
    out = np.zeros(128, np.uint8)
    oo = np.zeros(1, np.uint64)
    oc = np.array([128], np.uint32)
    olen = np.zeros(1, np.uint32)
    st = np.zeros(1, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)     # noqa: E731
    NULL = C.c_void_p(0)

    def call(n=1, mem=_lib.MEM_HOST, d=p(dic), dlen=len(dic), **over):
        a = dict(in_off=p(io), in_len=p(il), out_off=p(oo), out_cap=p(oc), out_len=p(olen), status=p(st))
        a.update(over)
        return lib.lz4flex_compress_batch_shared_dict(None, p(src), a["in_off"], a["in_len"], n, p(out), a["out_off"], a["out_cap"],
                                                      a["out_len"], a["status"], d, dlen, mem, None)

    for name in ("in_off", "in_len", "out_off", "out_cap", "out_len", "status"):
        assert call(**{name: NULL}) == -_lib.E_INVALID_ARG, name
    assert call(d=NULL, dlen=5) == -_lib.E_INVALID_ARG                       # a length without a dictionary
    assert call(mem=7) == -_lib.E_INVALID_ARG
    assert call(mem=_lib.MEM_DEVICE | _lib.MEM_CHAINED) == -_lib.E_INVALID_ARG
    assert call(mem=_lib.MEM_HOST | _lib.MEM_CHAINED) == -_lib.E_INVALID_ARG
    assert call(n=0) == 0
    assert call(n=0, in_off=NULL, status=NULL) == 0
    if lib.lz4flex_device_count() == 0:
        assert call() == -_lib.E_NO_DEVICE
        assert call(d=NULL, dlen=0) == -_lib.E_NO_DEVICE                      # (lz4flex_compress_batch without flags)
        assert call(mem=_lib.MEM_DEVICE) == -_lib.E_NO_DEVICE
        with pytest.raises(block.DeviceError):
            block.compress_batch_with_shared_dict(src, [0], [len(src)], dic, out, [0], [128])
        assert olen[0] == 0 and st[0] == 0 and not out.any()


def test_debug_counter_key_is_a_test_hook():
    """the digest counter is read through a debug_ key: refused without LZ4FLEX_TEST_HOOKS=1, like every other one"""
    import sys
    code = ("from lz4_flex_amd import _lib as L\nlib = L.load()\n"
            "r = lib.lz4flex_get_tuning(None, b'debug_shared_dict_items')\n"
            "print('RC', r)\n")
    env = {k: v for k, v in os.environ.items() if k != "LZ4FLEX_TEST_HOOKS"}
    out = subprocess.check_output([sys.executable, "-c", code], cwd=ROOT, env=env).decode()
    from lz4_flex_amd import _lib
    assert "RC %d" % -_lib.E_INVALID_ARG in out, out
