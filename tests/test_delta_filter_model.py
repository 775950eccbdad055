"""CPU test of the delta stage of typed batches: the numpy model of tests/delta_filter_model.py against the worked lines of
include/lz4flex_amd.h and its own inverse, and the lane-local helpers of lz4_flex_amd/csrc/lz4_filter_delta.h -- what the kernels of
lz4_filter.hip run on a lane's 16 elements, compiled for the host by tests/sim/filter_delta_shim.cpp -- against the model."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import delta_filter_model as D
import filter_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sim", "filter_delta_shim.cpp")
HDR = os.path.join(ROOT, "lz4_flex_amd", "csrc", "lz4_filter_delta.h")
SO = os.path.join(ROOT, "tests", "sim", "libfilter_delta_shim.so")
COUNTS = [0, 1, 2, 15, 16, 17, 1023, 1024, 1025, 1027, 1031, 2049, 3089, 65536]

_m = None


def shim():
    global _m
    if _m is None:
        if not os.path.exists(SO) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(SO):
            subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-Wall", SRC, "-o", SO])
        m = C.CDLL(SO)
        m.fd_delta16.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32]
        m.fd_scan16.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        m.fd_restart_index.argtypes = [C.c_uint64]
        for name in ("fd_restart_index", "fd_restart", "fd_add8", "fd_sub8", "fd_add16", "fd_sub16"):
            getattr(m, name).restype = C.c_uint32
        for name in ("fd_add8", "fd_sub8", "fd_add16", "fd_sub16"):
            getattr(m, name).argtypes = [C.c_uint32, C.c_uint32]
        _m = m
    return _m


def patterns(E, n, rnd):
    """n elements of E bytes as uint8: random, all 0xFF, monotone, and the carry patterns of each E"""
    u = D.UINT[E]
    out = [rnd.integers(0, 256, n * E, dtype=np.uint8), np.full(n * E, 0xFF, np.uint8),
           (np.cumsum(rnd.integers(0, 200, n)).astype(np.uint64) * np.uint64(3)).astype(u).view(np.uint8)]
    alt = {8: (0x00000000FFFFFFFF, 0x0000000100000000), 4: (0x0000FFFF, 0x00010000), 2: (0x00FF, 0x0100), 1: (0x7F, 0x80, 0xFF)}[E]
    out.append(np.resize(np.array(alt, np.uint64), n).astype(u).view(np.uint8))
    return out


def test_the_worked_lines_of_the_header():
    x = np.array([0x01, 0x00, 0x03, 0x00, 0x02, 0x00, 0xAA], np.uint8)
    want = np.array([0x01, 0x00, 0x02, 0x00, 0xFF, 0xFF, 0xAA], np.uint8)
    assert (D.delta(x, 2) == want).all() and (D.forward(x, M.NONE, 2) == want).all() and (D.undelta(want, 2) == x).all()
    y = D.delta(np.full(1026, 5, np.uint8), 1)
    assert y[0] == 5 and (y[1:1024] == 0).all() and y[1024] == 5 and y[1025] == 0 and y.size == 1026
    assert (D.forward(np.full(1026, 5, np.uint8), M.SHUFFLE, 1) == y).all()      # DELTA | SHUFFLE with E = 1 is the delta alone
    text = open(os.path.join(ROOT, "include", "lz4flex_amd.h")).read()
    assert "`01 00 03 00 02 00 AA` becomes `01 00 02 00 FF FF AA`" in text and "5, then 1 023 zeros, then 5, then 0" in text


@pytest.mark.parametrize("E", M.ELEMS)
@pytest.mark.parametrize("base", [M.NONE, M.SHUFFLE, M.BITSHUFFLE])
def test_inverse_of_forward_is_the_identity(base, E):
    rnd = np.random.default_rng(10 * base + E)
    for m in COUNTS:
        for tail in sorted({0, E - 1}):
            for x in patterns(E, m, rnd)[:2 if m > 4096 else 4]:
                x = np.concatenate([x, rnd.integers(0, 256, tail, dtype=np.uint8)])
                y = D.forward(x, base, E)
                assert y.size == x.size and (D.inverse(y, base, E) == x).all(), (base, E, m, tail)
                assert (y == M.forward(D.delta(x, E), base, E)).all()
                assert (D.forward(x, base, E, False) == M.forward(x, base, E)).all()
                if tail:
                    assert (y[m * E:] == x[m * E:]).all()
    for n in range(E):                                   # lengths below E: nothing to difference
        x = rnd.integers(0, 256, n, dtype=np.uint8)
        assert (D.forward(x, base, E) == x).all() and (D.inverse(x, base, E) == x).all()


@pytest.mark.parametrize("E", M.ELEMS)
def test_wrap_around_and_the_restart_at_1024(E):
    u, top = D.UINT[E], (1 << (8 * E)) - 1
    x = np.array([0, top, 0, 1, top - 1], np.uint64).astype(u)
    d = D.delta(x.view(np.uint8), E).view(u)
    assert [int(v) for v in d] == [0, top, 1, 1, top - 2]            # 0 - top = 1, (top - 1) - 1 = top - 2, all mod 2^(8 E)
    assert (D.undelta(d.view(np.uint8), E).view(u) == x).all()
    # a constant column: zero everywhere but at multiples of 1 024
    n = 3 * 1024 + 7
    d = D.delta(np.full(n, 0x5A, np.uint8).repeat(E), E).view(u)
    at = np.nonzero(d)[0]
    assert list(at) == [0, 1024, 2048, 3072] and D.RESTART == 1024
    # the bit-shuffle's residue is differenced like the rest: m = 1027, the restart at 1024 lies in it
    x = np.arange(1, 1028, dtype=np.uint64).astype(u)
    y = D.forward(x.view(np.uint8), M.BITSHUFFLE, E)
    assert [int(v) for v in y[1024 * E:].view(u)] == [1025 & top, 1, 1]
    x = x[:1023]
    assert [int(v) for v in D.forward(x.view(np.uint8), M.BITSHUFFLE, E)[1016 * E:].view(u)] == [1] * 7


def test_the_swar_adds_keep_their_fields_apart():
    m = shim()
    rnd = np.random.default_rng(7)
    edge = [0, 0xFFFFFFFF, 0x80808080, 0x7F7F7F7F, 0x00FF00FF, 0xFF00FF00, 0x01000100, 0x80008000, 0x7FFF7FFF, 0x0100FFFF]
    pairs = [(a, b) for a in edge for b in edge] + [tuple(int(v) for v in rnd.integers(0, 1 << 32, 2)) for _ in range(2000)]
    for a, b in pairs:
        a8, b8 = np.array([a], np.uint32).view(np.uint8), np.array([b], np.uint32).view(np.uint8)
        assert m.fd_add8(a, b) == int((a8 + b8).view(np.uint32)[0]) and m.fd_sub8(a, b) == int((a8 - b8).view(np.uint32)[0]), (hex(a), hex(b))
        a16, b16 = a8.view(np.uint16), b8.view(np.uint16)
        assert m.fd_add16(a, b) == int((a16 + b16).view(np.uint32)[0]) and m.fd_sub16(a, b) == int((a16 - b16).view(np.uint32)[0]), (hex(a), hex(b))


@pytest.mark.parametrize("E", M.ELEMS)
def test_lane_helpers_are_the_model(E):
    """a block of 4 096 + 16 elements cut into lanes of 16 at every phase h < 16 (a forward block's first aligned store lies up to 15
    elements in): delta16 with the element in front and the lane's restart index is the model's delta of those elements; scan16 + carry16
    with the sum of the elements back to the restart is the model's undelta (lanes that start a segment or lie inside one)"""
    m = shim()
    assert m.fd_restart() == D.RESTART
    u = D.UINT[E]
    rnd = np.random.default_rng(40 + E)
    for x in patterns(E, 4096 + 16, rnd):
        xv = x.view(u)
        d = D.delta(x, E)
        dv = d.view(u)
        for h in range(16):
            for e0 in list(range(h, 4096, 16))[::1 if h in (0, 5) else 7]:
                ri = m.fd_restart_index(e0)
                want_ri = [i for i in range(16) if (e0 + i) % 1024 == 0]
                assert ri == (want_ri[0] if want_ri else 16), (e0, ri)
                w = x[e0 * E:(e0 + 16) * E].copy()
                prev = int(xv[e0 - 1]) if e0 else 0xDEADBEEFDEADBEEF          # (block element 0 is a restart: prev is not looked at)
                assert m.fd_delta16(E, w.ctypes.data, prev, ri) == 0
                assert (w == d[e0 * E:(e0 + 16) * E]).all(), (E, e0, ri)
                if ri in (0, 16):                        # the inverse's lanes: 16-element aligned, a restart only at their first element
                    r = e0 - e0 % 1024
                    carry = int(np.sum(dv[r:e0], dtype=np.uint64)) if e0 > r else 0
                    w = d[e0 * E:(e0 + 16) * E].copy()
                    total = C.c_uint64(0)
                    assert m.fd_scan16(E, w.ctypes.data, carry, C.byref(total)) == 0
                    assert (w == x[e0 * E:(e0 + 16) * E]).all(), (E, e0)
                    mask = (1 << (8 * E)) - 1
                    assert total.value & mask == int(np.sum(dv[e0:e0 + 16], dtype=np.uint64)) & mask
    assert m.fd_delta16(3, None, 0, 0) == -1
