"""ctypes view of tests/sim/dict_train_model.c: the scalar definition of lz4flex_dict_train
(lz4_flex_amd/csrc/lz4_dict_train.hip).  Test infrastructure."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sim", "dict_train_model.c")
SO = os.path.join(ROOT, "tests", "sim", "libdict_train_model.so")
SEGMENT_DEFAULT = 512
E_UNSUPPORTED = 68

_m = None


def lib():
    global _m
    if _m is None:
        if not os.path.exists(SO) or os.path.getmtime(SRC) > os.path.getmtime(SO):
            subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-std=c11", "-Wall", SRC, "-o", SO])
        m = C.CDLL(SO)
        m.dtm_train.restype = C.c_int
        m.dtm_train.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_uint32)]
        _m = m
    return _m


def pack(samples, gap=0, lead=0):
    """the batch layout of a list of samples: (buffer u8, in_off u64, in_len u32), `lead` bytes in front and `gap` bytes between them"""
    lens = np.array([len(s) for s in samples], np.uint32)
    offs = np.zeros(len(samples), np.uint64)
    at = lead
    for i, s in enumerate(samples):
        offs[i] = at
        at += len(s) + gap
    buf = np.full(at + 1, 0xA5, np.uint8)
    for s, o in zip(samples, offs):
        buf[int(o):int(o) + len(s)] = np.frombuffer(bytes(s), np.uint8)
    return buf, offs, lens


def train_batch(buf, in_off, in_len, cap=32768, segment=SEGMENT_DEFAULT, with_picks=False):
    """(dictionary bytes, status) of the batch buf[in_off[i] : + in_len[i]]; with_picks: and the chosen segments, in the order of
    choice, as (sample, start, bytes taken)"""
    buf = np.ascontiguousarray(buf, np.uint8)
    offs, lens = np.ascontiguousarray(in_off, np.uint64), np.ascontiguousarray(in_len, np.uint32)
    k = segment or SEGMENT_DEFAULT
    out = np.zeros(max(cap, 1), np.uint8)
    picks = np.zeros(3 * 2 * ((cap + k - 1) // k) + 3, np.uint32)
    dl, st, npk = C.c_uint32(0), C.c_int32(0), C.c_uint32(0)
    rc = lib().dtm_train(buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, len(offs), out.ctypes.data, cap, segment,
                         C.byref(dl), C.byref(st), picks.ctypes.data, C.byref(npk))
    assert rc == 0, "the model ran out of memory"
    d = out[:dl.value].tobytes()
    if with_picks:
        return d, st.value, [tuple(int(v) for v in picks[3 * j:3 * j + 3]) for j in range(npk.value)]
    return d, st.value


def train(samples, cap=32768, segment=SEGMENT_DEFAULT, **kw):
    """train_batch of a list of bytes-likes laid out back to back"""
    buf, offs, lens = pack(samples)
    return train_batch(buf, offs, lens, cap, segment, **kw)
