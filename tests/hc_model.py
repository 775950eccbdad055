"""ctypes view of tests/sim/high_encoder_model.c: the scalar definition of compress_mode 2 ("high",
lz4_flex_amd/csrc/lz4_compress_high.hip).  Test infrastructure."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sim", "high_encoder_model.c")
SO = os.path.join(ROOT, "tests", "sim", "libhigh_encoder_model.so")
DEPTH_DEFAULT = 16       # "compress_depth"

_m = None


def lib():
    global _m
    if _m is None:
        if not os.path.exists(SO) or os.path.getmtime(SRC) > os.path.getmtime(SO):
            subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-std=c11", "-Wall", SRC, "-o", SO])
        m = C.CDLL(SO)
        m.lz4h_compress.restype = C.c_size_t
        m.lz4h_compress.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32]
        _m = m
    return _m


def compress(data, depth=DEPTH_DEFAULT):
    """the block compress_mode 2 writes for `data` at "compress_depth" `depth`"""
    data = bytes(data)
    assert 1 <= depth <= 256
    out = C.create_string_buffer(20 + len(data) * 110 // 100)
    n = lib().lz4h_compress(data, len(data), out, depth)
    return out.raw[:n]


def walk(comp):
    """the sequences of a block as (literals, match length) pairs; the last pair's match length is 0"""
    i, out = 0, []
    while True:
        t = comp[i]; i += 1
        lit = t >> 4
        if lit == 15:
            while True:
                b = comp[i]; i += 1; lit += b
                if b != 255:
                    break
        i += lit
        if i >= len(comp):
            out.append((lit, 0))
            return out
        i += 2
        ml = (t & 15) + 4
        if (t & 15) == 15:
            while True:
                b = comp[i]; i += 1; ml += b
                if b != 255:
                    break
        out.append((lit, ml))
