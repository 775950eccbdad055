"""CPU tests of the decompressed-size query (lz4flex_decompressed_size_batch): the Python model of the size walk (tests/size_model.py)
equals the oracle's decompress_internal with an unbounded sink on every corpus the GPU tests use, with and without history; and the C ABI
declares and exports the entry point, which needs a device (no CPU fallback)."""
import os
import re
import subprocess

import numpy as np
import pytest

import corpus
import ext_cases
import oracle_api as O
import size_model as S
from lz4_writer import Writer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_size(c, history=0, dict_form=False):
    """(status, size) from the oracle: decompress_internal with room for anything the block can produce"""
    cap = 255 * len(c) + 64
    if history == 0:
        st, r = O.decompress(c, cap)
    elif dict_form:
        st, r = O.decompress(c, cap, dict_data=bytes(history))
    else:
        st, r = O.decompress_prefix(c, bytes(history), history + cap)
    if st == "ok":
        return 0, len(r)
    assert st != "OutputTooSmall", "the capacity must never be the limit"
    return {v: k for k, v in S.NAMES.items()}[st], 0


def check(c, history=0):
    m = S.size(c, history)
    assert m == oracle_size(c, history), (m, len(c), history)
    if history:
        assert m == oracle_size(c, history, dict_form=True)
    return m


def test_model_adversarial_corpus():
    seen = set()
    for c, _cap in corpus.adversarial_blocks():
        seen.add(check(c)[0])
    assert seen == {0, S.LITERAL_OUT_OF_BOUNDS, S.EXPECTED_ANOTHER_BYTE, S.OFFSET_ZERO, S.OFFSET_OUT_OF_BOUNDS}, seen


def test_model_synthetic_blocks():
    for c, plain in corpus.synthetic_blocks():
        assert check(c) == (0, len(plain))


@pytest.mark.parametrize("p", ext_cases.PREFIX_LENS)
def test_model_writer_blocks_with_history(p):
    prefix = ext_cases.prefix_bytes(p)
    for name, c, new in ext_cases.writer_blocks(prefix):
        st, n = check(c, p)
        if new is not None:
            assert (st, n) == (0, len(new)), name
        check(c, 0)


def test_model_hand_written_blocks():
    statuses = {check(c, hist)[0] for _name, c, hist in S.writer_cases()}
    assert statuses == {0, S.EXPECTED_ANOTHER_BYTE, S.OFFSET_OUT_OF_BOUNDS}, statuses
    big = S.writer_cases()[0][1]
    assert len(big) < 4200 and S.size(big) == (0, (1 << 20) + 6)


def test_model_history_boundary():
    for hist in (0, 1, 7, 65530):
        for lit in (0, 1, 4):
            if hist + lit == 0:
                continue
            w = Writer(9, bytes(hist)).seq(lit, hist + lit, 4)
            assert check(w.end(5)[0], hist) == (0, lit + 4 + 5)
            w = Writer(9, bytes(hist)).bad_seq(lit, hist + lit + 1, 4)
            assert check(w.end(5)[0], hist) == (S.OFFSET_OUT_OF_BOUNDS, 0)


def test_model_liblz4_blocks():
    for d in (b"", b"a", bytes(100000), O.fixture_plain("compression_65k"), O.fixture_plain("compression_66k_JSON")):
        c = O.c_compress(d)
        assert check(c) == (0, len(d))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_size_batch():
    src = open(os.path.join(ROOT, "include", "lz4flex_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+lz4flex_decompressed_size_batch\s*\(", src)


def test_library_exports_size_batch_and_needs_a_device():
    from lz4_flex_amd import _lib, block, build
    lib_path = build.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path]).decode()
    assert re.search(r" T lz4flex_decompressed_size_batch\b", out)
    assert "lz4flex_decompressed_size_batch" in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.lz4flex_abi_version() >= 7
    c = O.compress(b"hello hello hello hello")
    if lib.lz4flex_device_count() == 0:
        with pytest.raises(block.DeviceError):
            block.decompressed_size_batch(np.frombuffer(c, np.uint8), [0], [len(c)])
        import ctypes as C
        size = np.zeros(1, np.uint64)
        st = np.zeros(1, np.int32)
        buf = np.frombuffer(c, np.uint8)
        rc = lib.lz4flex_decompressed_size_batch(None, C.c_void_p(buf.ctypes.data), C.c_void_p(np.array([0], np.uint64).ctypes.data),
                                                 C.c_void_p(np.array([len(c)], np.uint32).ctypes.data), 1, None,
                                                 C.c_void_p(size.ctypes.data), C.c_void_p(st.ctypes.data), _lib.MEM_HOST, None)
        assert rc == -_lib.E_NO_DEVICE
    else:
        size, st = block.decompressed_size_batch(np.frombuffer(c, np.uint8), [0], [len(c)])
        assert int(st[0]) == 0 and int(size[0]) == 23
