"""ctypes view of tests/sim/wave_encoder_model.c: the scalar model of the throughput ("wave") encoder
(lz4_flex_amd/csrc/lz4_compress_wave.hip).  Test infrastructure."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sim", "wave_encoder_model.c")
SO = os.path.join(ROOT, "tests", "sim", "libwave_encoder_model.so")
NSEG, CAP, SKIPD = 11, 1024, 64    # the kernel's constants (lz4_compress_wave.hip: WORKERS, CAP, SKIPD)


class Params(C.Structure):
    _fields_ = [("nseg", C.c_uint32), ("cap", C.c_uint32), ("skipd", C.c_uint32), ("hist", C.c_uint32), ("slide", C.c_uint32), ("sub", C.c_uint32)]


_m = None


def lib():
    global _m
    if _m is None:
        if not os.path.exists(SO) or os.path.getmtime(SRC) > os.path.getmtime(SO):
            subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-std=c11", "-Wall", SRC, "-o", SO])
        m = C.CDLL(SO)
        m.lz4w_compress.restype = C.c_size_t
        m.lz4w_compress.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.POINTER(Params), C.POINTER(C.c_uint32)]
        m.lz4w_trace.restype = C.c_size_t
        m.lz4w_trace.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        _m = m
    return _m


HIST = 32768                      # lz4_compress_wave.hip: HIST


SLIDE_DEFAULT = 2        # "compress_sliding_window": 0 = windows advance by 64 KiB, 1 = by 32 KiB, 2 = by 48 KiB (the default since round 5)


def auto_sub(n_blocks, workgroups):
    """what the library's default ("compress_subwindows" 0) picks for a batch of n_blocks with `workgroups` persistent workgroups
    (lz4flex_get_tuning "compress_workgroups")"""
    return 4 if n_blocks * 4 <= workgroups else (3 if n_blocks * 3 <= workgroups else (2 if n_blocks * 2 <= workgroups else 1))


def _params(n, nseg, cap, skipd, hist, slide, sub):
    if slide is None:           # the library's default ("compress_sliding_window" 2): the windows of a block longer than 64 KiB advance by 48 KiB (1: by 32 KiB)
        slide = SLIDE_DEFAULT if n - hist > 65536 else 0
    if sub is None:             # the library's default for a block that travels alone (a scalar call: auto_sub(1, ...) = 4); a block of a batch: auto_sub(n, workgroups)
        sub = 4
    return Params(nseg, cap, skipd, hist, slide, sub)


# lz4w_seq / lz4w_seg of wave_encoder_model.c (lz4w_trace)
SEQ_DTYPE = np.dtype([(f, np.uint32) for f in ("lit_start", "lit_len", "off", "mlen", "win", "wj", "first", "pend", "lane", "call", "run")])
SEG_DTYPE = np.dtype([(f, np.uint32) for f in ("win", "wj", "wbase", "s0", "s1", "run")])


def trace(data, nseg=NSEG, cap=CAP, skipd=SKIPD, hist=0, slide=None, sub=None):
    """the sequences compress() writes, in order, and where the kernel writes each (lz4w_trace): a record array of SEQ_DTYPE
    (positions count the history in front of the block; the last record is the final literals, mlen == 0), and the block's
    non-empty segments, a record array of SEG_DTYPE.  Same arguments as compress()."""
    data = bytes(data)
    assert hist == 0 or (hist == HIST and len(data) > hist)
    p = _params(len(data), nseg, cap, skipd, hist, slide, sub)
    seqs = np.zeros(len(data) // 4 + 2, dtype=SEQ_DTYPE)
    seg_cap = (len(data) // 16384 + 4) * nseg
    segs = np.zeros(seg_cap, dtype=SEG_DTYPE)
    nsg = C.c_size_t(0)
    ns = lib().lz4w_trace(data, len(data), C.byref(p), seqs.ctypes.data, segs.ctypes.data, seg_cap, C.byref(nsg))
    return seqs[:ns].copy(), segs[:nsg.value].copy()


def serialise(data, seqs):
    """the LZ4 block of a trace (compress.rs:237-247,463-486): what compress() must return"""
    data = bytes(data)
    if len(seqs) == 0:
        return b"\0"
    out = bytearray()

    def put_len(r):
        while r >= 255:
            out.append(255)
            r -= 255
        out.append(r)

    for s in seqs:
        lit, ml = int(s["lit_len"]), int(s["mlen"])
        out.append((min(lit, 15) << 4) | (min(ml - 4, 15) if ml else 0))
        if lit >= 15:
            put_len(lit - 15)
        out += data[int(s["lit_start"]):int(s["lit_start"]) + lit]
        if ml == 0:
            break
        out += int(s["off"]).to_bytes(2, "little")
        if ml - 4 >= 15:
            put_len(ml - 4 - 15)
    return bytes(out)


def compress(data, nseg=NSEG, cap=CAP, skipd=SKIPD, hist=0, slide=None, sub=None):
    """sub: 1, or 2 / 4 = sub-windows (what the library does to the blocks of small batches: auto_sub); slide: None = the library's default; hist: 0, or HIST -- `data` starts with HIST bytes of history (the stream in front of the block: a Linked frame), which are
    not emitted; the result is the block alone and needs them as its dictionary"""
    data = bytes(data)
    assert hist == 0 or (hist == HIST and len(data) > hist)
    out = C.create_string_buffer(20 + len(data) * 110 // 100 + 16)
    p = _params(len(data), nseg, cap, skipd, hist, slide, sub)
    ns = C.c_uint32(0)
    n = lib().lz4w_compress(data, len(data), out, C.byref(p), C.byref(ns))
    return out.raw[:n]
