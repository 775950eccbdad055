"""CPU: lz4flex_decompress_batch_partial_shared_dict, lz4flex_decompress_batch_partial_dict_set and
lz4flex_decompress_partial_into_with_dict -- the symbols, their bindings, and the argument checks that need no device: a wrong call is
refused before a device is looked for, an empty batch has nothing to do, a well-formed call without a device says NO_DEVICE."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lz4flex_amd.h")
SHARED = "lz4flex_decompress_batch_partial_shared_dict"
SET = "lz4flex_decompress_batch_partial_dict_set"
SCALAR = "lz4flex_decompress_partial_into_with_dict"
PYTHON = ["decompress_partial_with_dict", "decompress_batch_partial_with_shared_dict", "decompress_batch_partial_with_dict_set",
          "decompress_blocks_partial_with_shared_dict_device", "decompress_blocks_partial_with_dict_set_device"]


def _params(src, res, name):
    m = re.search(r"\b" + res + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
    assert m, name + " is not declared"
    return [p.split()[-1].lstrip("*") for p in m.group(1).split(",")]


def test_the_entries_are_declared_exported_and_bound():
    from lz4_flex_amd import _lib, block, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert _params(src, "int", SHARED) == ["ctx", "in_base", "in_off", "in_len", "n", "out_base", "out_off", "target", "out_len", "status",
                                          "dict", "dict_len", "mem_kind", "hip_stream"]
    assert _params(src, "int", SET) == ["ctx", "in_base", "in_off", "in_len", "n", "dict_id", "out_base", "out_off", "target", "out_len",
                                       "status", "set", "mem_kind", "hip_stream"]
    assert _params(src, "int64_t", SCALAR) == ["in", "in_len", "out", "target", "dict", "dict_len", "detail"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()]).decode()
    for name in (SHARED, SET, SCALAR):
        assert re.search(r" T " + name + r"\b", out), name
    V, U, I, Z = C.c_void_p, C.c_uint32, C.c_int, C.c_size_t
    assert _lib.SIGNATURES[SHARED] == (I, [V, V, V, V, U, V, V, V, V, V, V, U, I, V])
    assert _lib.SIGNATURES[SET] == (I, [V, V, V, V, U, V, V, V, V, V, V, V, I, V])
    res, args = _lib.SIGNATURES[SCALAR]
    assert res is C.c_int64 and args[:6] == [V, Z, V, Z, V, Z] and len(args) == 7
    for name in PYTHON:
        assert callable(getattr(block, name)), name
    # new symbols only: the number stays, and the version note names them
    assert _lib.load().lz4flex_abi_version() == 8
    note = open(HEADER).read().split("int lz4flex_abi_version")[0]
    assert all(name in note for name in (SHARED, SET, SCALAR))


class Args:
    """a well-formed one-block batch in host memory, a dictionary, and a pointer that stands for a set (never followed: every call that
    takes it is refused before the set is looked at, or has n == 0)"""

    def __init__(self):
        self.src = np.frombuffer(b"\x50hello", np.uint8).copy()
        self.off = np.zeros(1, np.uint64)
        self.len = np.array([6], np.uint32)
        self.out = np.zeros(128, np.uint8)
        self.target = np.array([3], np.uint32)
        self.ids = np.zeros(1, np.uint32)
        self.out_len = np.zeros(1, np.uint32)
        self.status = np.zeros(1, np.int32)
        self.dict = np.arange(32, dtype=np.uint8)

    def call(self, lib, entry, n=1, mem=0, drop=(), dict_len=32, set_=True):
        p = lambda a: C.c_void_p(a.ctypes.data)     # noqa: E731
        a = dict(in_off=p(self.off), in_len=p(self.len), dict_id=p(self.ids), out_off=p(self.off), target=p(self.target),
                 out_len=p(self.out_len), status=p(self.status), dict=p(self.dict))
        for name in ([drop] if isinstance(drop, str) else drop):
            a[name] = None
        if entry == "shared":
            return getattr(lib, SHARED)(None, p(self.src), a["in_off"], a["in_len"], n, p(self.out), a["out_off"], a["target"], a["out_len"],
                                        a["status"], a["dict"], dict_len, mem, None)
        return getattr(lib, SET)(None, p(self.src), a["in_off"], a["in_len"], n, a["dict_id"], p(self.out), a["out_off"], a["target"],
                                 a["out_len"], a["status"], p(self.src) if set_ else None, mem, None)


@pytest.fixture(scope="module")
def L():
    from lz4_flex_amd import _lib
    _lib.load()
    return _lib


ENTRIES = ["shared", "set"]


ARRAYS = ["in_off", "in_len", "out_off", "target", "out_len", "status"]


@pytest.mark.parametrize("entry,drop", [("shared", d) for d in ARRAYS] + [("set", d) for d in ARRAYS + ["dict_id"]])
def test_a_missing_array_is_refused(L, entry, drop):
    assert Args().call(L.load(), entry, drop=drop) == -L.E_INVALID_ARG


def test_a_missing_set_or_dictionary_is_refused(L):
    lib = L.load()
    assert Args().call(lib, "set", set_=False) == -L.E_INVALID_ARG
    assert Args().call(lib, "shared", drop="dict") == -L.E_INVALID_ARG            # NULL with dict_len != 0
    assert Args().call(lib, "shared", drop="dict", n=0) == -L.E_INVALID_ARG       # (before n is looked at)
    p = C.c_void_p(Args().src.ctypes.data)
    assert getattr(lib, SCALAR)(p, 6, p, 3, None, 5, None) == -L.E_INVALID_ARG
    assert getattr(lib, SCALAR)(p, 6, p, 1 << 32, p, 5, None) == -L.E_INVALID_ARG
    assert getattr(lib, SCALAR)(p, 6, p, 3, p, 1 << 32, None) == -L.E_INVALID_ARG


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_wrong_mem_kind_is_refused(L, entry):
    lib = L.load()
    for mem in (7, 0x1001, L.MEM_DEVICE | L.MEM_CHAINED, L.MEM_HOST | L.MEM_CHAINED, L.MEM_DEVICE | L.MEM_BIG_BLOCKS | L.MEM_CHAINED):
        a = Args()
        assert a.call(lib, entry, mem=mem) == -L.E_INVALID_ARG, hex(mem)
        assert a.call(lib, entry, n=0, mem=mem) == -L.E_INVALID_ARG, hex(mem)      # (the memory kind is looked at before n)


@pytest.mark.parametrize("entry", ENTRIES)
def test_an_empty_batch_has_nothing_to_do(L, entry):
    lib, a = L.load(), Args()
    assert a.call(lib, entry, n=0) == 0
    assert a.call(lib, entry, n=0, drop=("in_off", "status", "target", "dict_id"), set_=False) == 0
    assert a.call(lib, entry, n=0, mem=L.MEM_DEVICE | L.MEM_BIG_BLOCKS) == 0
    assert a.call(lib, entry, n=0, mem=L.MEM_HOST | L.MEM_BIG_BLOCKS) == 0


def test_without_a_device_a_well_formed_call_says_so(L):
    from lz4_flex_amd import block
    lib = L.load()
    if lib.lz4flex_device_count() != 0:
        return                                                # (a device is present: tests/test_gpu_partial_dict.py runs these calls)
    a = Args()
    for mem in (L.MEM_HOST, L.MEM_DEVICE, L.MEM_HOST | L.MEM_BIG_BLOCKS, L.MEM_DEVICE | L.MEM_BIG_BLOCKS):
        assert a.call(lib, "shared", mem=mem) == -L.E_NO_DEVICE, hex(mem)
        assert a.call(lib, "shared", mem=mem, dict_len=0) == -L.E_NO_DEVICE, hex(mem)          # (forwarded to the plain partial entry)
        assert a.call(lib, "shared", mem=mem, dict_len=0, drop="dict") == -L.E_NO_DEVICE, hex(mem)
        assert a.call(lib, "set", mem=mem) == -L.E_NO_DEVICE, hex(mem)
    p = lambda x: C.c_void_p(x.ctypes.data)     # noqa: E731
    assert getattr(lib, SCALAR)(p(a.src), 6, p(a.out), 3, p(a.dict), 32, None) == -L.E_NO_DEVICE
    assert getattr(lib, SCALAR)(p(a.src), 6, p(a.out), 3, None, 0, None) == -L.E_NO_DEVICE
    with pytest.raises(block.DeviceError):
        block.decompress_partial_with_dict(a.src.tobytes(), 3, a.dict.tobytes())
    with pytest.raises(block.DeviceError):
        block.decompress_batch_partial_with_shared_dict(a.src, [0], [6], a.dict, a.out, [0], [3])
    with pytest.raises(block.DeviceError):
        block.DictSet([a.dict.tobytes()])
    assert a.out_len[0] == 0 and a.status[0] == 0 and not a.out.any()
