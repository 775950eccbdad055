"""CPU: "compress_high_dict" and "compress_high_digest" -- compress_mode 2 ("high") against dictionaries: the settings and the Python
setter, as far as they need no device."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lz4flex_amd.h")
KEYS = ((b"compress_high_dict", 0), (b"compress_high_digest", 1))      # the key and its default


def test_the_keys_are_known_settings():
    """a known key answers with a context (or, without a device, with -E_NO_DEVICE: the default context); an unknown one is refused"""
    from lz4_flex_amd import _lib
    lib = _lib.load()
    for key, default in KEYS:
        assert lib.lz4flex_get_tuning(None, key + b"_") == -_lib.E_INVALID_ARG
        if lib.lz4flex_device_count() == 0:
            assert lib.lz4flex_get_tuning(None, key) == -_lib.E_NO_DEVICE
            assert lib.lz4flex_set_tuning(None, key, 1) == -_lib.E_NO_DEVICE
        else:
            ctx = C.c_void_p()
            assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
            try:
                assert lib.lz4flex_get_tuning(ctx, key) == default
                for v, rc in ((1, 0), (0, 0), (2, -_lib.E_INVALID_ARG), (-1, -_lib.E_INVALID_ARG)):
                    assert lib.lz4flex_set_tuning(ctx, key, v) == rc, (key, v)
                assert lib.lz4flex_get_tuning(ctx, key) == 0
            finally:
                lib.lz4flex_ctx_destroy(ctx)
        # the key is in the library and in the header's settings paragraph
        assert key + b"\0" in open(_lib.LIB_PATH, "rb").read()
        assert open(HEADER).read().count('"%s"' % key.decode()) >= 2
    # new settings only: no new symbol, the number stays
    assert lib.lz4flex_abi_version() == 8


def test_python_setter(monkeypatch):
    """block.set_compress_high_dict is "compress_high_dict" 0 / 1"""
    from lz4_flex_amd import _lib, block
    calls = []

    class Lib:
        def lz4flex_set_tuning(self, ctx, key, value):
            calls.append((ctx, key, value))
            return 0

    monkeypatch.setattr(_lib, "load", lambda: Lib())
    block.set_compress_high_dict(True)
    block.set_compress_high_dict(False, ctx=7)
    block.set_compress_high_dict(1)
    assert calls == [(None, b"compress_high_dict", 1), (7, b"compress_high_dict", 0), (None, b"compress_high_dict", 1)]
