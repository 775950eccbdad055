"""CPU: the dictionary-set entry points (lz4flex_dict_set_*, lz4flex_compress_batch_dict_set, lz4flex_decompress_batch_dict_set) answer
a wrong call before they look for a device -- the order of checks the header promises -- and say NO_DEVICE where the call is right and
no device exists.  No GPU is needed: every call here either is refused for its arguments or has nothing to do."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from lz4_flex_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NO_DEVICE = -L.E_INVALID_ARG, -L.E_NO_DEVICE


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _p(a):
    return C.c_void_p(a.ctypes.data)


class Args:
    """a well-formed one-block batch in host memory and a pointer that stands for a set (never followed: every call that takes it is
    refused before the set is looked at, or has n == 0)"""

    def __init__(self):
        self.buf = np.zeros(64, np.uint8)
        self.off = np.zeros(1, np.uint64)
        self.len = np.full(1, 8, np.uint32)
        self.cap = np.full(1, 40, np.uint32)
        self.ids = np.zeros(1, np.uint32)
        self.out_len = np.zeros(1, np.uint32)
        self.status = np.zeros(1, np.int32)
        self.detail = np.zeros(2, np.uint64)
        self.set = C.c_void_p(self.buf.ctypes.data)

    def call(self, lib, entry, n=1, mem=L.MEM_HOST, drop=None, set_=True):
        a = dict(in_off=_p(self.off), in_len=_p(self.len), dict_id=_p(self.ids), out_off=_p(self.off), out_cap=_p(self.cap),
                 out_len=_p(self.out_len), status=_p(self.status))
        if drop:
            a[drop] = None
        st = self.set if set_ else None
        if entry == "compress":
            return lib.lz4flex_compress_batch_dict_set(None, _p(self.buf), a["in_off"], a["in_len"], n, a["dict_id"], _p(self.buf), a["out_off"],
                                                       a["out_cap"], a["out_len"], a["status"], st, mem, None)
        return lib.lz4flex_decompress_batch_dict_set(None, _p(self.buf), a["in_off"], a["in_len"], n, a["dict_id"], _p(self.buf), a["out_off"],
                                                     a["out_cap"], a["out_len"], a["status"], _p(self.detail), st, mem, None)


ENTRIES = ["compress", "decompress"]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("drop", ["in_off", "in_len", "dict_id", "out_off", "out_cap", "out_len", "status"])
def test_a_missing_array_is_refused(lib, entry, drop):
    assert Args().call(lib, entry, drop=drop) == INVALID


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_missing_set_is_refused(lib, entry):
    assert Args().call(lib, entry, set_=False) == INVALID


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("mem", [7, L.MEM_DEVICE | L.MEM_CHAINED, L.MEM_HOST | L.MEM_CHAINED])
def test_a_wrong_mem_kind_is_refused(lib, entry, mem):
    a = Args()
    assert a.call(lib, entry, mem=mem) == INVALID
    assert a.call(lib, entry, n=0, mem=mem) == INVALID      # (the memory kind is looked at before n)


@pytest.mark.parametrize("entry", ENTRIES)
def test_an_empty_batch_has_nothing_to_do(lib, entry):
    a = Args()
    assert a.call(lib, entry, n=0) == 0
    assert a.call(lib, entry, n=0, set_=False) == 0
    assert a.call(lib, entry, n=0, mem=L.MEM_DEVICE | L.MEM_BIG_BLOCKS, drop="dict_id") == 0


def _create(lib, k, off=True, length=True, out=True, mem=L.MEM_HOST):
    d = np.zeros(16, np.uint8)
    offs = np.zeros(max(k, 1), np.uint64)
    lens = np.full(max(k, 1), 4, np.uint32)
    h = C.c_void_p(1)
    rc = lib.lz4flex_dict_set_create(None, _p(d), _p(offs) if off else None, _p(lens) if length else None, k, mem, C.byref(h) if out else None)
    return rc, h


def test_create_checks_its_arguments_first(lib):
    for k in (0, 1025, 0xFFFFFFFF):
        rc, h = _create(lib, k)
        assert rc == INVALID and not h.value, k
    assert _create(lib, 2, off=False)[0] == INVALID
    assert _create(lib, 2, length=False)[0] == INVALID
    assert _create(lib, 2, out=False)[0] == INVALID
    assert _create(lib, 2, mem=7)[0] == INVALID
    assert _create(lib, 2, mem=L.MEM_HOST | L.MEM_BIG_BLOCKS)[0] == INVALID


def test_create_without_a_device_says_so(lib):
    if lib.lz4flex_device_count() > 0:
        rc, h = _create(lib, 2)
        assert rc == 0 and h.value
        assert lib.lz4flex_dict_set_count(h) == 2
        lib.lz4flex_dict_set_free(h)
    else:
        for k in (1, 1024):
            rc, h = _create(lib, k)
            assert rc == NO_DEVICE and not h.value


def test_free_and_count_of_nothing(lib):
    lib.lz4flex_dict_set_free(None)
    assert lib.lz4flex_dict_set_count(None) == 0


def test_the_abi_version_stays(lib):
    assert lib.lz4flex_abi_version() == 8


def test_the_counter_key_is_a_test_hook():
    """"debug_dict_set_items" is refused in a process that has not opted in (before a device is looked for), and cannot be set"""
    code = ("import ctypes as C\nfrom lz4_flex_amd import _lib as L\nlib = L.load()\n"
            "print(lib.lz4flex_get_tuning(None, b'debug_dict_set_items'), lib.lz4flex_set_tuning(None, b'debug_dict_set_items', 1))")
    env = {k: v for k, v in os.environ.items() if k != "LZ4FLEX_TEST_HOOKS"}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.split() == [str(INVALID).encode()] * 2
    # with the hooks on the key is read-only: setting it is refused before a device is looked for
    assert L.load().lz4flex_set_tuning(None, b"debug_dict_set_items", 1) == INVALID
