"""CPU: compress_mode 2 ("high") and "compress_depth" -- the settings and their Python and command-line forms, as far as they need no
device."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lz4flex_amd.h")


def test_compress_depth_is_a_known_setting():
    """a known key answers with a context (or, without a device, with -E_NO_DEVICE: the default context); an unknown one is refused"""
    from lz4_flex_amd import _lib
    lib = _lib.load()
    assert lib.lz4flex_get_tuning(None, b"compress_depth_") == -_lib.E_INVALID_ARG
    if lib.lz4flex_device_count() == 0:
        assert lib.lz4flex_get_tuning(None, b"compress_depth") == -_lib.E_NO_DEVICE
        assert lib.lz4flex_set_tuning(None, b"compress_depth", 16) == -_lib.E_NO_DEVICE
        assert lib.lz4flex_set_tuning(None, b"compress_mode", 2) == -_lib.E_NO_DEVICE
    else:
        ctx = C.c_void_p()
        assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
        try:
            assert lib.lz4flex_get_tuning(ctx, b"compress_depth") == 16
            for v, rc in ((1, 0), (256, 0), (0, -_lib.E_INVALID_ARG), (257, -_lib.E_INVALID_ARG), (-1, -_lib.E_INVALID_ARG)):
                assert lib.lz4flex_set_tuning(ctx, b"compress_depth", v) == rc, v
            assert lib.lz4flex_get_tuning(ctx, b"compress_depth") == 256
            assert lib.lz4flex_set_tuning(ctx, b"compress_mode", 2) == 0 and lib.lz4flex_get_tuning(ctx, b"compress_mode") == 2
            assert lib.lz4flex_set_tuning(ctx, b"compress_mode", 3) == -_lib.E_INVALID_ARG
        finally:
            lib.lz4flex_ctx_destroy(ctx)
    # the key is in the library and in the header's settings paragraph; new settings only: the number stays
    assert b"compress_depth\0" in open(_lib.LIB_PATH, "rb").read()
    assert open(HEADER).read().count('"compress_depth"') >= 2
    assert lib.lz4flex_abi_version() == 8


def test_python_names_of_the_mode(monkeypatch):
    """block.set_compress_mode("high") is "compress_mode" 2, block.set_compress_depth is "compress_depth"; an unknown name is refused"""
    from lz4_flex_amd import _lib, block
    calls = []

    class Lib:
        def lz4flex_set_tuning(self, ctx, key, value):
            calls.append((ctx, key, value))
            return 0

    monkeypatch.setattr(_lib, "load", lambda: Lib())
    block.set_compress_mode("high")
    block.set_compress_mode("fast", ctx=7)
    block.set_compress_depth(64)
    assert calls == [(None, b"compress_mode", 2), (7, b"compress_mode", 0), (None, b"compress_depth", 64)]
    with pytest.raises(KeyError):
        block.set_compress_mode("higher")


def test_command_line_flags():
    """--high / --depth go with a compression, --depth with --high and 1 .. 256: refused before anything is opened"""
    from lz4_flex_amd import cli
    for argv in (["--depth", "4"], ["--high", "--depth", "0"], ["--high", "--depth", "257"], ["--high", "-d"], ["--high", "x.lz4"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert isinstance(e.value.code, str), argv
