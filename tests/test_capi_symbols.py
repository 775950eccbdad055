"""CPU test: the C-ABI shared library loads and exports every symbol include/lz4flex_amd.h declares,
and fails loudly (no CPU fallback) when there is no GPU.  No compute calls."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lz4flex_amd.h")


@pytest.fixture(scope="module")
def lib_path():
    from lz4_flex_amd import build
    return build.build()   # hipcc cross-compiles gfx950 without a GPU


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(lz4flex_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_expected_entry_points():
    names = declared_functions()
    for must in ("lz4flex_compress_into", "lz4flex_decompress_into", "lz4flex_compress_batch", "lz4flex_decompress_batch",
                 "lz4flex_frame_encoder_new", "lz4flex_frame_decoder_new", "lz4flex_get_maximum_output_size"):
        assert must in names


def test_library_exports_every_declared_symbol(lib_path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path]).decode()
    exported = set(re.findall(r" T (lz4flex_[a-z0-9_]+)", out))
    missing = [n for n in declared_functions() if n not in exported]
    assert not missing, missing


def test_ctypes_binding_covers_header(lib_path):
    from lz4_flex_amd import _lib
    lib = _lib.load()
    for n in declared_functions():
        assert n in _lib.SIGNATURES, n
        assert getattr(lib, n) is not None


def test_library_contains_gfx950_code_object(lib_path):
    data = open(lib_path, "rb").read()
    assert b"gfx950" in data
    assert b"lz4_decompress_blocks_kernel" in data and b"lz4_compress_blocks_kernel" in data


def test_host_logic_without_gpu(lib_path):
    """pure host entry points work anywhere; compute entry points refuse to run without a device"""
    import ctypes as C
    from lz4_flex_amd import _lib, block, frame
    lib = _lib.load()
    assert block.get_maximum_output_size(65536) == 72109
    assert frame.FrameInfo(block_size=frame.BlockSize.Max64KB).write() == bytes([0x04, 0x22, 0x4D, 0x18, 0x60, 0x40, 0x82])
    assert frame.FrameInfo(block_size=frame.BlockSize.Max64KB, block_mode=frame.BlockMode.Linked).write()[-1] == 0xC0
    fi = frame.FrameInfo.read(bytes([0x04, 0x22, 0x4D, 0x18, 0x40, 0x40, 0xC0]))
    assert fi.block_mode == frame.BlockMode.Linked and fi.block_size == frame.BlockSize.Max64KB
    with pytest.raises(frame.HeaderChecksumError):
        frame.FrameInfo.read(bytes([0x04, 0x22, 0x4D, 0x18, 0x40, 0x40, 0xC1]))
    assert lib.lz4flex_xxh32(b"", 0, 0) == 0x02CC5D05
    if lib.lz4flex_device_count() == 0:
        with pytest.raises(block.DeviceError):
            block.compress(b"no gpu, no codec")
        with pytest.raises(block.DeviceError):
            block.decompress(bytes([0x10, 0x61]), 1)
        assert lib.lz4flex_get_tuning(None, b"compress_mode") == -_lib.E_NO_DEVICE      # the default context needs a device too
        assert lib.lz4flex_set_tuning(None, b"compress_mode", 1) == -_lib.E_NO_DEVICE


def test_stale_library_is_detected(lib_path):
    """the build is keyed on a hash of EVERY file under csrc/ and include/ (round 1 shipped a library that
    predated a header edit because a hand-kept dependency list missed it)"""
    from lz4_flex_amd import _lib, build
    assert not build.needs_build()
    assert _lib.load().lz4flex_build_id().decode() == build.source_hash()
    hdrs = [p for p in build.dep_files() if p.endswith(".h")]
    assert len(hdrs) >= 3
    for victim in hdrs:
        with open(victim, "rb") as f:
            orig = f.read()
        try:
            with open(victim, "ab") as f:
                f.write(b"\n// touched by test_stale_library_is_detected\n")
            assert build.needs_build(), victim
        finally:
            with open(victim, "wb") as f:
                f.write(orig)
    assert not build.needs_build()


def test_dispatch_thresholds_are_readable_without_a_device():
    """the decoder dispatch's batch-size table (lz4_device.h) through lz4flex_get_tuning: ascending, ends where the key is refused --
    tests/test_gpu_dispatch_matrix.py builds its size matrix from it"""
    from lz4_flex_amd import _lib
    lib = _lib.load()
    ts = []
    for i in range(32):
        v = lib.lz4flex_get_tuning(None, b"dispatch_threshold_%d" % i)
        if v < 0:
            break
        ts.append(v)
    assert len(ts) >= 5 and ts == sorted(ts) and ts[-1] == 16384
    assert lib.lz4flex_get_tuning(None, b"dispatch_threshold_x") < 0


def test_decoder_configurations_are_listed_without_a_device():
    """lz4flex_get_tuning "decoder_config_<i>": every decoder configuration the build can be pinned to (variant * 1000 + parameter); the
    GPU decoder matrix (tests/test_gpu_block.py DECODERS) and tools/gpu_fuzz.py are generated from it"""
    from lz4_flex_amd import _lib
    lib = _lib.load()
    cs = []
    for i in range(64):
        v = lib.lz4flex_get_tuning(None, b"decoder_config_%d" % i)
        if v < 0:
            break
        cs.append(v)
    assert {1016, 4064, 7000, 8000, 10000, 11000, 13000} <= set(cs) and len(cs) == len(set(cs))
    assert not ({9000, 12000} & set(cs))     # the plan / replay and the fused decoder left the product library (tools builds only)
    assert not ({5000, 6000} & set(cs))      # the wave decoder and its two-wavefront form: replaced by the sequence decoder (13) in round 6
    for gone in (5, 6, 9, 12):
        assert lib.lz4flex_set_tuning(None, b"decompress_variant", gone) < 0
    assert lib.lz4flex_get_tuning(None, b"decoder_config_") < 0


def test_many_frames_entry_points_check_their_arguments_without_a_device():
    """lz4flex_frame_{compress,decompress}_many: nothing to do is success, missing arrays are refused before any device is touched;
    with no device the calls fail loudly (there is no CPU path)"""
    import ctypes as C
    from lz4_flex_amd import _lib, frame
    lib = _lib.load()
    z = (C.c_uint64 * 1)(0)
    st = (C.c_int32 * 1)(0)
    buf = C.create_string_buffer(64)
    assert lib.lz4flex_frame_compress_many(None, buf, z, z, 0, None, buf, z, z, z, st, _lib.MEM_HOST, None) == 0
    assert lib.lz4flex_frame_decompress_many(None, buf, z, z, 0, buf, z, z, z, st, None, _lib.MEM_HOST, None) == 0
    assert lib.lz4flex_frame_compress_many(None, buf, None, z, 1, None, buf, z, z, z, st, _lib.MEM_HOST, None) == -_lib.E_INVALID_ARG
    assert lib.lz4flex_frame_decompress_many(None, buf, z, z, 1, buf, z, z, z, None, None, _lib.MEM_HOST, None) == -_lib.E_INVALID_ARG
    assert frame.compress_frames([]) == [] and frame.decompress_frames([], 10) == []
    if lib.lz4flex_device_count() == 0:
        cap = (C.c_uint64 * 1)(64)
        assert lib.lz4flex_frame_compress_many(None, buf, z, z, 1, None, buf, z, cap, z, st, _lib.MEM_HOST, None) == -_lib.E_NO_DEVICE
        from lz4_flex_amd import block
        with pytest.raises(block.DeviceError):
            frame.compress_frames([b"no gpu, no codec"])


def _one_block_args():
    """a valid 1-block host batch (one literal) as ctypes arrays: in, in_off, in_len, out, out_off, out_cap, out_len, status"""
    import ctypes as C
    return (C.create_string_buffer(bytes([0x10, 0x61]), 16), (C.c_uint64 * 1)(0), (C.c_uint32 * 1)(2), C.create_string_buffer(64),
            (C.c_uint64 * 1)(0), (C.c_uint32 * 1)(64), (C.c_uint32 * 1)(0), (C.c_int32 * 1)(0))


def test_batched_entry_points_keep_their_order_of_checks_and_mem_kinds(lib_path):
    """lz4flex_compress_batch / lz4flex_decompress_batch look for a context before they look at the arrays; the dictionary path of
    lz4flex_compress_batch_ex and both *_shared_dict entries check their arguments first and accept fewer mem_kind values (the table in
    capi.cpp's classify_mem calls).  Callers see both."""
    import ctypes as C
    from lz4_flex_amd import _lib
    lib = _lib.load()
    INV, NODEV = -_lib.E_INVALID_ARG, -_lib.E_NO_DEVICE
    have = lib.lz4flex_device_count() > 0
    src, in_off, in_len, out, out_off, cap, out_len, st = _one_block_args()
    dic = C.create_string_buffer(b"dictionary", 16)
    dlen = (C.c_uint32 * 1)(10)
    ext = _lib.CompressExt(C.cast(dic, C.c_void_p), C.cast(in_off, C.c_void_p), C.cast(dlen, C.c_void_p))

    def compress(mem, off=in_off):
        return lib.lz4flex_compress_batch(None, src, off, in_len, None, 1, out, out_off, cap, out_len, st, mem, None)

    def decompress(mem, off=in_off):
        return lib.lz4flex_decompress_batch(None, src, off, in_len, 1, out, out_off, cap, out_len, st, None, mem, None)

    def compress_ex(mem, off=in_off):
        return lib.lz4flex_compress_batch_ex(None, src, off, in_len, None, 1, out, out_off, cap, out_len, st, C.byref(ext), mem, None)

    def compress_shared(mem, off=in_off):
        return lib.lz4flex_compress_batch_shared_dict(None, src, off, in_len, 1, out, out_off, cap, out_len, st, dic, 10, mem, None)

    def decompress_shared(mem, off=in_off):
        return lib.lz4flex_decompress_batch_shared_dict(None, src, off, in_len, 1, out, out_off, cap, out_len, st, None, dic, 10, mem, None)

    if not have:
        assert compress(_lib.MEM_HOST, None) == NODEV and decompress(_lib.MEM_HOST, None) == NODEV
        assert compress(7) == NODEV and decompress(7) == NODEV
    for entry in (compress_ex, compress_shared, decompress_shared):
        assert entry(_lib.MEM_HOST, None) == INV, entry.__name__
        for mem in (7, _lib.MEM_DEVICE | _lib.MEM_CHAINED, 0x1001):
            assert entry(mem) == INV, (entry.__name__, hex(mem))
    assert compress_ex(_lib.MEM_HOST | _lib.MEM_BIG_BLOCKS) == INV and compress_shared(_lib.MEM_HOST | _lib.MEM_BIG_BLOCKS) == INV
    # accepted: the call goes on to its context (and, with a device, decodes the block)
    st[0], out_len[0] = -1, 99
    assert decompress_shared(_lib.MEM_HOST | _lib.MEM_BIG_BLOCKS) == (0 if have else NODEV)
    if have:
        assert (st[0], out_len[0], out.raw[:1]) == (0, 1, b"a")
    else:
        assert (st[0], out_len[0]) == (-1, 99)
    assert compress_ex(_lib.MEM_HOST) == (0 if have else NODEV) and compress_shared(_lib.MEM_HOST) == (0 if have else NODEV)


SETTINGS = ["decompress_lanes", "compress_mode", "compress_subwindows", "compress_deterministic", "decompress_level_chains",
            "decompress_blocks_per_wg", "decompress_variant", "decompress_second_pass", "decompress_pcd_pair", "compress_carry_wait",
            "compress_sliding_window", "compress_variant", "compress_lanes", "size_scan_serial", "compress_shared_dict",
            "decompress_shared_dict"]
HOOKS = ["debug_chain_giveup", "debug_fail_next_batch", "debug_exact_dict_piece"]            # set only
READ_ONLY = ["compress_workgroups", "debug_shared_dict_items"]     # (dispatch_threshold_<i>, decoder_config_<i>: the two tests above)


def test_every_settings_key_without_a_context(lib_path):
    """lz4flex_set_tuning / lz4flex_get_tuning with a NULL context: an unknown key is refused as such on any machine, a known one goes
    on to the default context -- which needs a device; the test hooks do not exist in a process that has not asked for them"""
    import sys
    from lz4_flex_amd import _lib
    lib = _lib.load()
    INV, NODEV = -_lib.E_INVALID_ARG, -_lib.E_NO_DEVICE
    assert os.environ.get("LZ4FLEX_TEST_HOOKS") == "1"
    for key in ("no_such_key", "", "debug_no_such_hook", "compress_mode_", "Compress_mode"):
        assert lib.lz4flex_set_tuning(None, key.encode(), 0) == INV, key
        assert lib.lz4flex_get_tuning(None, key.encode()) == INV, key
    assert lib.lz4flex_set_tuning(None, None, 0) == INV and lib.lz4flex_get_tuning(None, None) == INV
    assert lib.lz4flex_set_tuning(None, b"debug_shared_dict_items", 0) == INV
    if lib.lz4flex_device_count() == 0:
        for key in SETTINGS + HOOKS + READ_ONLY:
            assert lib.lz4flex_get_tuning(None, key.encode()) == NODEV, key
        for key in SETTINGS + HOOKS + READ_ONLY[:1]:
            assert lib.lz4flex_set_tuning(None, key.encode(), 1) == NODEV, key
    # without LZ4FLEX_TEST_HOOKS=1 every "debug_" key is refused before a context is looked for
    env = {k: v for k, v in os.environ.items() if k != "LZ4FLEX_TEST_HOOKS"}
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from lz4_flex_amd import _lib\n"
            "lib = _lib.load()\n"
            "for k in %r:\n"
            "    assert lib.lz4flex_set_tuning(None, k.encode(), 0) == -_lib.E_INVALID_ARG, k\n"
            "    assert lib.lz4flex_get_tuning(None, k.encode()) == -_lib.E_INVALID_ARG, k\n" % (ROOT, HOOKS + ["debug_shared_dict_items"]))
    subprocess.check_call([sys.executable, "-c", code], env=env)
