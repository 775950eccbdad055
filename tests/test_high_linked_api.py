"""CPU: "compress_high_linked" -- compress_mode 2 ("high") over a stream's history: the setting, its environment variable, the Python
setter and the command line's --linked, as far as they need no device."""
import ctypes as C
import io
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lz4flex_amd.h")
KEY = b"compress_high_linked"


def test_the_key_is_a_known_setting():
    """a known key answers with a context (or, without a device, with -E_NO_DEVICE: the default context); an unknown one is refused"""
    from lz4_flex_amd import _lib
    lib = _lib.load()
    assert lib.lz4flex_get_tuning(None, KEY + b"_") == -_lib.E_INVALID_ARG
    if lib.lz4flex_device_count() == 0:
        assert lib.lz4flex_get_tuning(None, KEY) == -_lib.E_NO_DEVICE
        assert lib.lz4flex_set_tuning(None, KEY, 1) == -_lib.E_NO_DEVICE
    else:
        ctx = C.c_void_p()
        assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
        try:
            assert lib.lz4flex_get_tuning(ctx, KEY) == 0
            for v, rc in ((1, 0), (0, 0), (2, -_lib.E_INVALID_ARG), (-1, -_lib.E_INVALID_ARG)):
                assert lib.lz4flex_set_tuning(ctx, KEY, v) == rc, v
            assert lib.lz4flex_get_tuning(ctx, KEY) == 0
        finally:
            lib.lz4flex_ctx_destroy(ctx)
    # the key and its environment variable are in the library, the key in the header's settings paragraph
    binary = open(_lib.LIB_PATH, "rb").read()
    assert KEY + b"\0" in binary and b"LZ4FLEX_HIGH_LINKED\0" in binary
    assert open(HEADER).read().count('"%s"' % KEY.decode()) >= 2
    # a new setting only: no new symbol, the number stays
    assert lib.lz4flex_abi_version() == 8


@pytest.mark.gpu
def test_the_environment_variable():
    """LZ4FLEX_HIGH_LINKED=1 is a new context's "compress_high_linked" (a fresh process: the variable is read when a context is made)"""
    code = ("import ctypes as C\nfrom lz4_flex_amd import _lib\nlib = _lib.load()\nctx = C.c_void_p()\n"
            "assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0\nprint(lib.lz4flex_get_tuning(ctx, b'compress_high_linked'))\n")
    for value, want in (("1", "1"), (None, "0")):
        env = dict(os.environ, PYTHONPATH=ROOT)
        env.pop("LZ4FLEX_HIGH_LINKED", None)
        if value is not None:
            env["LZ4FLEX_HIGH_LINKED"] = value
        assert subprocess.check_output([sys.executable, "-c", code], env=env, cwd=ROOT).decode().strip() == want, value


def test_python_setter(monkeypatch):
    """block.set_compress_high_linked is "compress_high_linked" 0 / 1"""
    from lz4_flex_amd import _lib, block
    calls = []

    class Lib:
        def lz4flex_set_tuning(self, ctx, key, value):
            calls.append((ctx, key, value))
            return 0

    monkeypatch.setattr(_lib, "load", lambda: Lib())
    block.set_compress_high_linked(True)
    block.set_compress_high_linked(False, ctx=7)
    block.set_compress_high_linked(1)
    assert calls == [(None, KEY, 1), (7, KEY, 0), (None, KEY, 1)]


def test_cli_linked_option(monkeypatch, tmp_path):
    """--linked asks for BlockMode.Linked; --high --linked turns the setting on, --high alone leaves it off"""
    from lz4_flex_amd import block, cli, frame
    seen = []

    class Enc:
        def __init__(self, wtr, frame_info=None):
            seen.append(("encoder", frame_info.block_mode if frame_info else None))

        new = classmethod(lambda cls, wtr: cls(wtr))
        with_frame_info = classmethod(lambda cls, fi, wtr: cls(wtr, fi))

        def write(self, b):
            return len(b)

        def finish(self):
            pass

    monkeypatch.setattr(cli, "FrameEncoder", Enc)
    monkeypatch.setattr(block, "set_compress_mode", lambda m: seen.append(("mode", m)))
    monkeypatch.setattr(block, "set_compress_high_linked", lambda on: seen.append(("linked", bool(on))))
    src = tmp_path / "a.txt"
    src.write_bytes(b"abc" * 100)
    out = str(tmp_path / "a.lz4")
    cli.main([str(src), "-f", "-o", out, "--high", "--linked"])
    cli.main([str(src), "-f", "-o", out, "--linked"])
    cli.main([str(src), "-f", "-o", out, "--high"])
    assert seen == [("mode", "high"), ("linked", True), ("encoder", frame.BlockMode.Linked),
                    ("encoder", frame.BlockMode.Linked),
                    ("mode", "high"), ("linked", False), ("encoder", None)]
    with pytest.raises(SystemExit):
        cli.main([out, "-f", "--linked"])
    # standard input to a file: the same choice
    del seen[:]
    monkeypatch.setattr(cli.sys, "stdin", type("In", (), {"buffer": io.BytesIO(b"abc" * 100)})())
    cli.main(["-o", out, "--linked"])
    monkeypatch.setattr(cli.sys, "stdin", type("In", (), {"buffer": io.BytesIO(b"abc" * 100)})())
    cli.main(["-o", out])
    assert seen == [("encoder", frame.BlockMode.Linked), ("encoder", None)]
