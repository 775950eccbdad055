"""ctypes view of tests/sim/high_optimal_model.c: the scalar definition of compress_mode 2 ("high") under "compress_parse" 1, the optimal
parse over the unchanged best[] (lz4_flex_amd/csrc/lz4_compress_high.hip, step 3 1/2).  Test infrastructure."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM = os.path.join(ROOT, "tests", "sim")
SRC = os.path.join(SIM, "high_optimal_model.c")
BASES = [os.path.join(SIM, "high_dict_model.c"), os.path.join(SIM, "high_encoder_model.c")]      # (included by SRC)
SO = os.path.join(SIM, "libhigh_optimal_model.so")
DEPTH_DEFAULT = 16       # "compress_depth"
HISTORY = 32768          # what the definition reads of a dictionary or of the bytes in front of a block
SEGMENT = 2048           # the parse's segments: positions of a chunk that are priced together
SHORT_MAX = 35           # the longest length below the full one that is priced

_m = None
_memo = {}


def lib():
    global _m
    if _m is None:
        if not os.path.exists(SO) or max(os.path.getmtime(f) for f in [SRC] + BASES) > os.path.getmtime(SO):
            subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-std=c11", "-Wall", SRC, "-o", SO])
        m = C.CDLL(SO)
        m.lz4ho_compress.restype = C.c_size_t
        m.lz4ho_compress.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32]
        m.lz4ho_compress_trace.restype = C.c_size_t
        m.lz4ho_compress_trace.argtypes = m.lz4ho_compress.argtypes + [C.POINTER(C.c_uint32)] * 3
        _m = m
    return _m


def compress(data, dict_data=b"", depth=DEPTH_DEFAULT, parse=1):
    """the block compress_mode 2 writes for `data` against `dict_data` (with "compress_high_dict" 1, or as its history with
    "compress_high_linked" 1) at "compress_depth" `depth` and "compress_parse" `parse`"""
    data, dict_data = bytes(data), bytes(dict_data)
    assert 1 <= depth <= 256 and parse in (0, 1)
    key = (data, dict_data, depth, parse)
    if key not in _memo:
        out = C.create_string_buffer(20 + len(data) * 110 // 100)
        n = lib().lz4ho_compress(data, len(data), dict_data, len(dict_data), out, depth, parse)
        _memo[key] = out.raw[:n]
    return _memo[key]


def trace(data, dict_data=b"", depth=DEPTH_DEFAULT, parse=1):
    """(block, best[].len, best[].off, the length the walk reads) -- a list entry per position of `data`"""
    data, dict_data = bytes(data), bytes(dict_data)
    out = C.create_string_buffer(20 + len(data) * 110 // 100)
    arr = [(C.c_uint32 * max(len(data), 1))() for _ in range(3)]
    n = lib().lz4ho_compress_trace(data, len(data), dict_data, len(dict_data), out, depth, parse, *arr)
    return (out.raw[:n],) + tuple(list(a)[:len(data)] for a in arr)


def block(stream, at, n, h, depth=DEPTH_DEFAULT, parse=1):
    """the bytes of stream[at : at + n] with the h bytes in front of it as its history (tests/hc_linked_model.py's block)"""
    assert 0 <= h <= at
    hist = bytes(stream[at - min(h, HISTORY):at]) if h >= 4 else b""
    return compress(stream[at:at + n], hist, depth, parse)
