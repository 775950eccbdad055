"""CPU: the seekable-frame entries (lz4flex_frame_index_* and lz4flex_frame_read_ranges) -- the symbols and their bindings, the argument
checks that need no device, the two settings, and what a machine without a device answers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_index_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lz4flex_amd.h")
ENTRIES = ["lz4flex_frame_index_create", "lz4flex_frame_index_free", "lz4flex_frame_index_blocks", "lz4flex_frame_index_content_size",
           "lz4flex_frame_index_frame_bytes", "lz4flex_frame_index_info", "lz4flex_frame_index_table", "lz4flex_frame_read_ranges"]
KEYS = ["frame_range_pass_bytes", "frame_range_checksums"]


def _params(ret, name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
    assert m, name + " is not declared"
    return [p.split()[-1].lstrip("*") for p in m.group(1).split(",")]


def test_entries_are_declared_exported_and_bound():
    from lz4_flex_amd import _lib, build, frame
    assert _params("int", ENTRIES[0]) == ["ctx", "frame", "frame_len", "mem_kind", "out", "detail"]
    assert _params("int", ENTRIES[7]) == ["ctx", "x", "frame", "range_off", "range_len", "m", "out_base", "out_off", "out_len", "status", "detail",
                                          "mem_kind", "hip_stream"]
    assert _params("int", ENTRIES[6]) == ["x", "content_off", "payload_off", "len_word"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()]).decode()
    for name in ENTRIES:
        assert re.search(r" T " + name + r"\b", out), name
        assert name in _lib.SIGNATURES, name
    V, U, I, U64 = C.c_void_p, C.c_uint32, C.c_int, C.c_uint64
    assert _lib.SIGNATURES[ENTRIES[7]] == (I, [V, V, V, V, V, U, V, V, V, V, V, I, V])
    assert _lib.SIGNATURES[ENTRIES[0]][1][:4] == [V, V, U64, I]
    assert _lib.SIGNATURES[ENTRIES[2]][0] is U and _lib.SIGNATURES[ENTRIES[3]][0] is U64 and _lib.SIGNATURES[ENTRIES[4]][0] is U64
    for name in ("FrameIndex", "read_ranges_device"):
        assert callable(getattr(frame, name))
    for name in ("blocks", "content_size", "frame_bytes", "frame_info", "table", "read", "read_ranges"):
        assert hasattr(frame.FrameIndex, name)
    # new symbols only: the number stays, callers detect them by the symbol
    assert _lib.load().lz4flex_abi_version() == 8
    note = open(HEADER).read().split("int lz4flex_abi_version")[0]
    assert "lz4flex_frame_index_create" in note and "lz4flex_frame_read_ranges" in note and all('"%s"' % k in note for k in KEYS)


def test_argument_checks_need_no_device():
    from lz4_flex_amd import _lib, block, frame
    lib = _lib.load()
    w = FC.seven()
    buf = np.frombuffer(w.frame, np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)     # noqa: E731
    NULL = C.c_void_p(0)
    h = C.c_void_p(0x1234)
    d = _lib.ErrDetail()
    create = lib.lz4flex_frame_index_create
    assert create(None, p(buf), len(buf), _lib.MEM_HOST, None, C.byref(d)) == -_lib.E_INVALID_ARG
    assert create(None, NULL, len(buf), _lib.MEM_HOST, C.byref(h), None) == -_lib.E_INVALID_ARG and h.value is None   # (*out is cleared)
    for mem in (7, _lib.MEM_HOST | _lib.MEM_BIG_BLOCKS, _lib.MEM_DEVICE | _lib.MEM_CHAINED):
        assert create(None, p(buf), len(buf), mem, C.byref(h), None) == -_lib.E_INVALID_ARG, hex(mem)
    # the accessors of no index are harmless
    lib.lz4flex_frame_index_free(None)
    assert lib.lz4flex_frame_index_blocks(None) == 0 and lib.lz4flex_frame_index_content_size(None) == 0
    assert lib.lz4flex_frame_index_frame_bytes(None) == 0 and lib.lz4flex_frame_index_table(None, None, None, None) == -_lib.E_INVALID_ARG
    ro, rl, oo = np.zeros(1, np.uint64), np.ones(1, np.uint64), np.zeros(1, np.uint64)
    ol, st, out = np.zeros(1, np.uint64), np.zeros(1, np.int32), np.zeros(64, np.uint8)
    read = lib.lz4flex_frame_read_ranges
    # x == NULL, whatever else is right -- and also with m == 0
    for m in (0, 1):
        assert read(None, None, p(buf), p(ro), p(rl), m, p(out), p(oo), p(ol), p(st), None, _lib.MEM_HOST, None) == -_lib.E_INVALID_ARG
    if lib.lz4flex_device_count() == 0:
        assert create(None, p(buf), len(buf), _lib.MEM_HOST, C.byref(h), C.byref(d)) == -_lib.E_NO_DEVICE and h.value is None
        assert create(None, p(buf), len(buf), _lib.MEM_DEVICE, C.byref(h), None) == -_lib.E_NO_DEVICE
        with pytest.raises(block.DeviceError):
            frame.FrameIndex(w.frame)
        return
    # with a device: the checks of read_ranges on a real index, before a context is looked at
    ix = frame.FrameIndex(w.frame)
    x = ix._h

    def call(m=1, mem=_lib.MEM_HOST, **over):
        a = dict(frame=p(buf), range_off=p(ro), range_len=p(rl), out_base=p(out), out_off=p(oo), out_len=p(ol), status=p(st))
        a.update(over)
        return read(None, x, a["frame"], a["range_off"], a["range_len"], m, a["out_base"], a["out_off"], a["out_len"], a["status"], None, mem, None)

    for name in ("frame", "range_off", "range_len", "out_base", "out_off", "out_len", "status"):
        assert call(**{name: NULL}) == -_lib.E_INVALID_ARG, name
    for mem in (7, _lib.MEM_HOST | _lib.MEM_BIG_BLOCKS, _lib.MEM_DEVICE | _lib.MEM_CHAINED):
        assert call(mem=mem) == -_lib.E_INVALID_ARG and call(m=0, mem=mem) == -_lib.E_INVALID_ARG
    assert call(m=0) == 0 and call(m=0, range_off=NULL, status=NULL, out_base=NULL) == 0
    assert call() == 0 and st[0] == 0 and ol[0] == 1 and bytes(out[:2]) == w.content[:1] + b"\0"
    ix.close()


def test_the_two_settings():
    from lz4_flex_amd import _lib
    lib = _lib.load()
    for key in KEYS:
        assert lib.lz4flex_get_tuning(None, (key + "_").encode()) == -_lib.E_INVALID_ARG
        assert (key + "\0").encode() in open(_lib.LIB_PATH, "rb").read()
        assert open(HEADER).read().count('"%s"' % key) >= 2
    if lib.lz4flex_device_count() == 0:
        for key in KEYS:
            assert lib.lz4flex_get_tuning(None, key.encode()) == -_lib.E_NO_DEVICE
            assert lib.lz4flex_set_tuning(None, key.encode(), 1) == -_lib.E_NO_DEVICE
        return
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
    try:
        assert lib.lz4flex_get_tuning(ctx, b"frame_range_pass_bytes") == 256 << 20
        assert lib.lz4flex_set_tuning(ctx, b"frame_range_pass_bytes", 1) == 0 and lib.lz4flex_get_tuning(ctx, b"frame_range_pass_bytes") == 1
        assert lib.lz4flex_set_tuning(ctx, b"frame_range_pass_bytes", 0) == -_lib.E_INVALID_ARG
        assert lib.lz4flex_get_tuning(ctx, b"frame_range_checksums") == 1
        assert lib.lz4flex_set_tuning(ctx, b"frame_range_checksums", 0) == 0 and lib.lz4flex_get_tuning(ctx, b"frame_range_checksums") == 0
        assert lib.lz4flex_set_tuning(ctx, b"frame_range_checksums", 2) == -_lib.E_INVALID_ARG
    finally:
        lib.lz4flex_ctx_destroy(ctx)
