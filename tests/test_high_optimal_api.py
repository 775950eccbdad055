"""CPU: "compress_parse" -- the setting and its Python, environment and command-line forms, as far as they need no device."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lz4flex_amd.h")


def test_compress_parse_is_a_known_setting():
    """a known key answers with a context (or, without a device, with -E_NO_DEVICE: the default context); it takes 0 and 1"""
    from lz4_flex_amd import _lib
    lib = _lib.load()
    assert lib.lz4flex_get_tuning(None, b"compress_parse_") == -_lib.E_INVALID_ARG
    if lib.lz4flex_device_count() == 0:
        assert lib.lz4flex_get_tuning(None, b"compress_parse") == -_lib.E_NO_DEVICE
        assert lib.lz4flex_set_tuning(None, b"compress_parse", 1) == -_lib.E_NO_DEVICE
    else:
        ctx = C.c_void_p()
        assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
        try:
            assert lib.lz4flex_get_tuning(ctx, b"compress_parse") == 0
            for v, rc in ((1, 0), (0, 0), (1, 0), (2, -_lib.E_INVALID_ARG), (-1, -_lib.E_INVALID_ARG)):
                assert lib.lz4flex_set_tuning(ctx, b"compress_parse", v) == rc, v
            assert lib.lz4flex_get_tuning(ctx, b"compress_parse") == 1
            # it is a setting of mode 2, not a mode
            assert lib.lz4flex_set_tuning(ctx, b"compress_mode", 3) == -_lib.E_INVALID_ARG
        finally:
            lib.lz4flex_ctx_destroy(ctx)
    image = open(_lib.LIB_PATH, "rb").read()
    assert b"compress_parse\0" in image and b"LZ4FLEX_HIGH_PARSE\0" in image
    # the settings paragraph and the list of later additions; a new setting only: the number stays
    assert open(HEADER).read().count('"compress_parse"') >= 2
    assert lib.lz4flex_abi_version() == 8


def test_python_names_of_the_parse(monkeypatch):
    from lz4_flex_amd import _lib, block
    calls = []

    class Lib:
        def lz4flex_set_tuning(self, ctx, key, value):
            calls.append((ctx, key, value))
            return 0

    monkeypatch.setattr(_lib, "load", lambda: Lib())
    block.set_compress_parse("optimal")
    block.set_compress_parse("lazy", ctx=7)
    assert calls == [(None, b"compress_parse", 1), (7, b"compress_parse", 0)]
    for name in ("best", 1, None):
        with pytest.raises(KeyError):
            block.set_compress_parse(name)
    assert len(calls) == 2


def test_command_line_flags():
    """--optimal goes with --high and with a compression: refused before anything is opened"""
    from lz4_flex_amd import cli
    for argv in (["--optimal"], ["--optimal", "--depth", "4"], ["--high", "--optimal", "-d"], ["--high", "--optimal", "x.lz4"], ["--optimal", "-d"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert isinstance(e.value.code, str), argv


def test_command_line_sets_the_parse(monkeypatch, tmp_path):
    """--high --optimal is set_compress_parse("optimal"); --high alone leaves the parse as the process has it"""
    from lz4_flex_amd import block, cli
    calls = []
    monkeypatch.setattr(block, "set_compress_mode", lambda m, ctx=None: calls.append(("mode", m)))
    monkeypatch.setattr(block, "set_compress_depth", lambda d, ctx=None: calls.append(("depth", d)))
    monkeypatch.setattr(block, "set_compress_parse", lambda p, ctx=None: calls.append(("parse", p)))
    monkeypatch.setattr(block, "set_compress_high_linked", lambda on, ctx=None: calls.append(("linked", on)))
    monkeypatch.setattr(cli, "handle_file", lambda *a, **k: calls.append(("file", a[0])))
    src = str(tmp_path / "in.txt")
    assert cli.main(["--high", "--optimal", "--depth", "64", src]) == 0
    assert cli.main(["--high", src]) == 0
    assert calls == [("mode", "high"), ("depth", 64), ("parse", "optimal"), ("linked", False), ("file", src),
                     ("mode", "high"), ("linked", False), ("file", src)]
