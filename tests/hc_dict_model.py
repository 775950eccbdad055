"""ctypes view of tests/sim/high_dict_model.c: the scalar definition of compress_mode 2 ("high") against an external dictionary
("compress_high_dict" 1; lz4_flex_amd/csrc/lz4_compress_high.hip, the dictionary form).  Test infrastructure."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sim", "high_dict_model.c")
BASE = os.path.join(ROOT, "tests", "sim", "high_encoder_model.c")      # (included by SRC)
SO = os.path.join(ROOT, "tests", "sim", "libhigh_dict_model.so")
DEPTH_DEFAULT = 16       # "compress_depth"

_m = None


def lib():
    global _m
    if _m is None:
        if not os.path.exists(SO) or max(os.path.getmtime(SRC), os.path.getmtime(BASE)) > os.path.getmtime(SO):
            subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-std=c11", "-Wall", SRC, "-o", SO])
        m = C.CDLL(SO)
        m.lz4h_compress_dict.restype = C.c_size_t
        m.lz4h_compress_dict.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32]
        _m = m
    return _m


def compress(data, dict_data=b"", depth=DEPTH_DEFAULT):
    """the block compress_mode 2 writes for `data` against `dict_data` at "compress_depth" `depth` with "compress_high_dict" 1"""
    data, dict_data = bytes(data), bytes(dict_data)
    assert 1 <= depth <= 256
    out = C.create_string_buffer(20 + len(data) * 110 // 100)
    n = lib().lz4h_compress_dict(data, len(data), dict_data, len(dict_data), out, depth)
    return out.raw[:n]
