"""GPU: the frame index (lz4flex_frame_index_create) and range reads through it (lz4flex_frame_read_ranges), both memory kinds.

The checker is never the code under test: the bytes of range (o, l) are full[o : o + l], `full` the oracle's frame_decompress of the same
frame; the tables are the Python writer's own positions (tests/frame_index_cases.py, held against the oracle on the CPU); a create
failure is the oracle's frame_decompress error for the same bytes; a damaged block read without its checksum is what the partial model
(tests/partial_model.py, pinned to the oracle) gives that block at the range's target.
Every output region lies between 64-byte canaries at an offset that is no multiple of 16, and the frame is compared with its copy."""
import ctypes as C
import io
import os
import random
import struct
import subprocess
import sys

import numpy as np
import pytest

import frame_index_cases as FC
import oracle_api as O
import partial_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5
HOST, DEVICE = 0, 1
FE_DECOMPRESSION, FE_IO, FE_BLOCK_CHECKSUM = 17, 18, 26
E_UNSUPPORTED = 68


@pytest.fixture(scope="module")
def fr():
    from lz4_flex_amd import _lib, frame
    assert _lib.load().lz4flex_device_count() >= 1
    return frame


@pytest.fixture(scope="module")
def frames():
    out = FC.all_frames()
    for w in out.values():
        rc, full, _ = O.frame_decompress(w.frame, len(w.content) + 64)
        assert rc == 0
        w.full = full                                    # the reference, computed once and left alone
    return out


@pytest.fixture
def tuning():
    """settings of the default context, put back afterwards"""
    from lz4_flex_amd import _lib
    lib, changed = _lib.load(), {}

    def set_(key, value):
        k = key.encode()
        changed.setdefault(k, lib.lz4flex_get_tuning(None, k))
        assert lib.lz4flex_set_tuning(None, k, value) == 0
    yield set_
    for k, v in changed.items():
        assert lib.lz4flex_set_tuning(None, k, v) == 0


def _u64(v):
    return np.array(list(v) or [0], np.uint64)


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _index(frame_bytes, mem):
    """(rc, handle, (expected, actual, inner), keep-alive)"""
    import torch
    from lz4_flex_amd import _lib
    lib = _lib.load()
    h, d = C.c_void_p(), _lib.ErrDetail()
    host = np.frombuffer(bytes(frame_bytes), np.uint8)
    if mem == DEVICE:
        dev = torch.from_numpy(host.copy()).cuda()
        rc = lib.lz4flex_frame_index_create(None, C.c_void_p(dev.data_ptr()), len(host), _lib.MEM_DEVICE, C.byref(h), C.byref(d))
    else:
        dev = None
        rc = lib.lz4flex_frame_index_create(None, _ptr(host), len(host), _lib.MEM_HOST, C.byref(h), C.byref(d))
    return rc, h, (int(d.expected), int(d.actual), int(d.inner)), dev


def _read(h, frame_bytes, ranges, mem, S):
    """[(status, bytes or None, (expected, actual, inner))]; asserts the canaries around every region, the untouched frame, and out_len"""
    import torch
    from lz4_flex_amd import _lib
    lib = _lib.load()
    m = len(ranges)
    want = [min(n, S - o) if o < S else 0 for o, n in ranges]
    out_off, at = [], 0
    for v in want:
        at += 64
        at += (5 - at) % 16                               # (no multiple of 16)
        out_off.append(at); at += v
    total = at + 64
    host_out = np.full(total, CANARY, np.uint8)
    host_in = np.frombuffer(bytes(frame_bytes), np.uint8).copy()
    ro, rl, oo = _u64(o for o, _ in ranges), _u64(n for _, n in ranges), _u64(out_off)
    ol, st, det = np.full(max(m, 1), 77, np.uint64), np.full(max(m, 1), 77, np.int32), (_lib.ErrDetail * max(m, 1))()
    if mem == DEVICE:
        d_in, d_out = torch.from_numpy(host_in).cuda(), torch.from_numpy(host_out).cuda()
        rc = lib.lz4flex_frame_read_ranges(None, h, C.c_void_p(d_in.data_ptr()), _ptr(ro), _ptr(rl), m, C.c_void_p(d_out.data_ptr()), _ptr(oo), _ptr(ol),
                                           _ptr(st), det, _lib.MEM_DEVICE, None)
        got, back = d_out.cpu().numpy(), d_in.cpu().numpy()
    else:
        rc = lib.lz4flex_frame_read_ranges(None, h, _ptr(host_in), _ptr(ro), _ptr(rl), m, _ptr(host_out), _ptr(oo), _ptr(ol), _ptr(st), det,
                                           _lib.MEM_HOST, None)
        got, back = host_out, host_in
    assert rc == 0, _lib.last_error()
    assert back.tobytes() == bytes(frame_bytes), "the frame was written to"
    mask = np.ones(total, bool)
    res = []
    for r in range(m):
        mask[out_off[r]:out_off[r] + want[r]] = False
        dt = (int(det[r].expected), int(det[r].actual), int(det[r].inner))
        if st[r] == 0:
            assert ol[r] == want[r], (ranges[r], int(ol[r]))
            res.append((0, got[out_off[r]:out_off[r] + want[r]].tobytes(), dt))
        else:
            assert ol[r] == 0, ranges[r]
            res.append((int(st[r]), None, dt))
    assert (got[mask] == CANARY).all(), "bytes outside the ranges' regions were written"
    return res


def _seven_ranges(w):
    co, S = w.content_off, w.content_off[-1]
    size = [b - a for a, b in zip(co, co[1:])]
    out = [(c + d, n) for c in co for d in (-1, 0, 1) for n in (0, 1, 2, 17) if c + d >= 0]
    out += [(co[b], size[b]) for b in range(len(size))]                                                    # each block alone
    out += [(co[b] + size[b] // 2, size[b] - size[b] // 2 + size[b + 1] // 2) for b in range(len(size) - 1)]   # middle to middle
    out += [(co[3] + 1000, 3000), (co[3] + 65535, 1), (0, S), (1, S), (S - 1, 5), (S, 5), (S + 10, 5), (co[1] + 7, co[6] - co[1])]
    out += [(co[1] + 1000 * i + 3, 500 + i) for i in range(40)]                                            # forty into the same block
    rnd = random.Random(5)
    out += [(rnd.randrange(S), rnd.choice([1, 100, 5000, 70000, 140000])) for _ in range(60)]
    return out


def _check_all(res, ranges, full):
    for (st, data, dt), (o, n) in zip(res, ranges):
        assert st == 0 and data == full[o:o + n] and dt == (0, 0, 0), (o, n, st, dt)


@pytest.mark.parametrize("mem", [HOST, DEVICE])
def test_index_contents(frames, mem):
    from lz4_flex_amd import _lib
    lib = _lib.load()
    for name, w in frames.items():
        rc, h, _, keep = _index(w.frame, mem)
        assert rc == 0, name
        n = len(w.len_word)
        assert lib.lz4flex_frame_index_blocks(h) == n and lib.lz4flex_frame_index_content_size(h) == len(w.full) == w.content_off[-1]
        assert lib.lz4flex_frame_index_frame_bytes(h) == len(w.frame), name
        co, po, lw = np.zeros(n + 1, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        assert lib.lz4flex_frame_index_table(h, _ptr(co), _ptr(po), _ptr(lw)) == 0
        assert (co.tolist(), po.tolist(), lw.tolist()) == (w.content_off, w.payload_off, w.len_word), name
        assert lib.lz4flex_frame_index_table(h, None, _ptr(po), None) == 0
        fi = _lib.FrameInfoC()
        lib.lz4flex_frame_index_info(h, C.byref(fi))
        assert (fi.block_size, fi.block_mode, bool(fi.block_checksums)) == (4, 0, w.block_checksums), name
        assert bool(fi.has_content_size) == ("sized" in name) and (not fi.has_content_size or fi.content_size == len(w.full))
        lib.lz4flex_frame_index_free(h)


@pytest.mark.parametrize("mem", [HOST, DEVICE])
@pytest.mark.parametrize("name", ["seven", "seven_sums"])
def test_ranges_of_the_seven_block_frame(frames, tuning, mem, name):
    from lz4_flex_amd import _lib
    w = frames[name]
    S = len(w.full)
    ranges = _seven_ranges(w)
    assert 200 < len(ranges) < 500
    rc, h, _, keep = _index(w.frame, mem)
    assert rc == 0
    try:
        first = _read(h, w.frame, ranges, mem, S)                          # ONE call
        _check_all(first, ranges, w.full)
        tuning("frame_range_pass_bytes", 1)                                # one range per pass (a head alone is over that budget)
        assert _read(h, w.frame, ranges, mem, S) == first
        tuning("frame_range_pass_bytes", 100000)
        assert _read(h, w.frame, ranges, mem, S) == first
        tuning("frame_range_pass_bytes", 256 << 20)
        tuning("decompress_partial", 0)                                    # every block in the reference's order
        assert _read(h, w.frame, ranges, mem, S) == first
    finally:
        _lib.load().lz4flex_frame_index_free(h)


@pytest.mark.parametrize("mem", [HOST, DEVICE])
@pytest.mark.parametrize("name", ["plain", "sized", "sums_sized"])
def test_ranges_of_the_other_frames(frames, mem, name):
    from lz4_flex_amd import _lib
    w = frames[name]
    S = len(w.full)
    rnd = random.Random(len(name))
    ranges = [(c + d, n) for c in w.content_off for d in (-1, 0, 1) for n in (1, 17, 65536) if c + d >= 0]
    ranges += [(0, S), (S - 1, 5), (S, 5), (0, 0)] + [(rnd.randrange(S), rnd.randrange(1, 200000)) for _ in range(50)]
    rc, h, _, keep = _index(w.frame, mem)
    assert rc == 0
    try:
        _check_all(_read(h, w.frame, ranges, mem, S), ranges, w.full)
    finally:
        _lib.load().lz4flex_frame_index_free(h)


def _touched(w, o, n):
    S = w.content_off[-1]
    n = min(n, S - o) if o < S else 0
    return [b for b in range(len(w.len_word)) if n and w.content_off[b] < o + n and w.content_off[b + 1] > o]


_partial_cache = {}


def _expected_without_checksums(w, damaged, o, n):
    """(status, bytes): block by block, a compressed block cut at the range's last byte in it by the partial model"""
    out = b""
    for b in _touched(w, o, n):
        c0, c1 = w.content_off[b], w.content_off[b + 1]
        lo, hi = max(o, c0), min(o + n, c1)
        pay = damaged[w.payload_off[b]:w.payload_off[b] + (w.len_word[b] & ~FC.STORED)]
        if w.len_word[b] & FC.STORED:
            out += pay[lo - c0:hi - c0]
            continue
        key = (pay, hi - c0)
        if key not in _partial_cache:
            _partial_cache[key] = partial_model.partial(pay, hi - c0)
        st, data = _partial_cache[key]
        if st != 0:
            return (-FE_DECOMPRESSION, st), None
        if len(data) != hi - c0:
            return (-FE_DECOMPRESSION, 0), None                            # (fewer bytes than the index says: inner 0)
        out += data[lo - c0:]
    return (0, 0), out


@pytest.mark.parametrize("mem", [HOST, DEVICE])
def test_block_checksums(frames, tuning, mem):
    from lz4_flex_amd import _lib
    w = frames["seven_sums"]
    S, co = len(w.full), w.content_off
    rc, h, _, keep = _index(w.frame, mem)
    assert rc == 0
    ranges = [(co[5] + 10, 100), (co[5], 1), (co[6] - 1, 1), (co[6] - 1, 2), (co[4], 20), (co[3] + 9, 70000), (0, S), (co[5] + 30000, 40000),
              (co[5], 65531), (co[5] + 65000, 531)]
    ranges += [(0, co[5]), (co[6], 40000), (co[4] + 1, 6), (co[1] + 5, 100), (co[6] + 77, 5), (0, 1)]
    try:
        for k in (3, 1000, (w.len_word[5] & ~FC.STORED) - 1):
            damaged = bytearray(w.frame)
            damaged[w.payload_off[5] + k] ^= 0x10
            damaged = bytes(damaged)
            tuning("frame_range_checksums", 1)
            res = _read(h, damaged, ranges, mem, S)
            hit = 0
            for (st, data, dt), (o, n) in zip(res, ranges):
                if 5 in _touched(w, o, n):
                    assert (st, data, dt) == (-FE_BLOCK_CHECKSUM, None, (0, 0, 0)), (o, n)
                    hit += 1
                else:
                    assert st == 0 and data == w.full[o:o + n], (o, n)
            assert hit == 10
            tuning("frame_range_checksums", 0)                             # the damaged block as the decoder sees it
            res = _read(h, damaged, ranges, mem, S)
            for (st, data, dt), (o, n) in zip(res, ranges):
                (want_st, inner), want = _expected_without_checksums(w, damaged, o, n)
                assert st == want_st and data == want and dt[2] == inner, (k, o, n, st, dt)
        # the stored 7-byte block's checksum word
        tuning("frame_range_checksums", 1)
        damaged = bytearray(w.frame)
        damaged[w.payload_off[4] + 7 + 2] ^= 0x80
        ranges = [(co[4] + 2, 3), (co[3] + 100, 50), (co[5], 10), (co[4] - 1, 1), (co[5] - 1, 2), (co[3] + 65000, 1000), (co[4], 7)]
        res = _read(h, bytes(damaged), ranges, mem, S)
        assert [st for st, _, _ in res] == [-FE_BLOCK_CHECKSUM, 0, 0, 0, -FE_BLOCK_CHECKSUM, -FE_BLOCK_CHECKSUM, -FE_BLOCK_CHECKSUM]
        for (st, data, _), (o, n) in zip(res, ranges):
            assert st != 0 or data == w.full[o:o + n]
    finally:
        _lib.load().lz4flex_frame_index_free(h)


@pytest.mark.parametrize("mem", [HOST, DEVICE])
def test_create_failures_are_the_decoders(mem):
    from lz4_flex_amd import _lib
    for name, f in FC.broken_frames().items():
        code, detail, _ = O.frame_decompress(f, 1 << 20)
        assert code != 0, name
        rc, h, d, keep = _index(f, mem)
        assert rc == -code and not h.value, (name, rc, code)
        assert d == detail, (name, d, detail)
    rc, h, d, keep = _index(FC.no_end_mark(), mem)
    assert rc == -FE_IO and not h.value
    rc, linked = O.frame_compress(FC.text()[:200000], block_mode=1, block_size=4)
    assert rc == 0
    legacy = struct.pack("<I", 0x184C2102) + struct.pack("<I", len(O.compress(b"a" * 100))) + O.compress(b"a" * 100)
    for f in (linked, legacy):
        rc, h, d, keep = _index(f, mem)
        assert rc == -E_UNSUPPORTED and not h.value


@pytest.mark.parametrize("mem", [HOST, DEVICE])
def test_a_second_frame_behind_the_first_is_ignored(frames, mem):
    from lz4_flex_amd import _lib
    lib = _lib.load()
    w = frames["sized"]
    both = w.frame + frames["seven"].frame
    rc, h, _, keep = _index(both, mem)
    assert rc == 0
    try:
        assert lib.lz4flex_frame_index_frame_bytes(h) == len(w.frame) and lib.lz4flex_frame_index_content_size(h) == len(w.full)
        ranges = [(0, len(w.full) + 99), (len(w.full) - 3, 99)]
        _check_all(_read(h, both, ranges, mem, len(w.full)), ranges, w.full)
    finally:
        lib.lz4flex_frame_index_free(h)


@pytest.mark.parametrize("mem", [HOST, DEVICE])
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_frames_of_the_librarys_own_encoder(fr, mem, mode):
    from lz4_flex_amd import _lib, block
    t, r = FC.text(), FC.rand()
    parts = [t[:100000], r[:3000], t[7:70007], t[:5], r[:65536] + t[:1000], t[1000:250000]]
    block.set_compress_mode(mode)
    try:
        buf = io.BytesIO()
        enc = fr.FrameEncoder.with_frame_info(fr.FrameInfo(block_size=fr.BlockSize.Max64KB, block_checksums=True), buf)
        for p in parts:
            enc.write(p)
            enc.flush()
        enc.finish()
    finally:
        block.set_compress_mode("fast")
    stream, frame_bytes = b"".join(parts), buf.getvalue()
    rnd = random.Random(9)
    ranges = [(rnd.randrange(len(stream)), rnd.choice([1, 50, 4096, 66000, 200000])) for _ in range(50)]
    rc, h, _, keep = _index(frame_bytes, mem)
    assert rc == 0
    try:
        assert _lib.load().lz4flex_frame_index_blocks(h) >= 9            # (flush boundaries: short blocks inside the frame)
        _check_all(_read(h, frame_bytes, ranges, mem, len(stream)), ranges, stream)
    finally:
        _lib.load().lz4flex_frame_index_free(h)


def test_python_interface(fr, frames, tmp_path):
    import torch
    w = frames["seven_sums"]
    S, co = len(w.full), w.content_off
    with fr.FrameIndex(w.frame) as ix:
        assert (ix.blocks, ix.content_size, ix.frame_bytes) == (7, S, len(w.frame))
        assert ix.table() == (w.content_off, w.payload_off, w.len_word)
        assert ix.frame_info.block_checksums and ix.frame_info.block_size == fr.BlockSize.Max64KB
        assert ix.read(co[1] + 9, 70000) == w.full[co[1] + 9:co[1] + 70009] and ix.read(S - 2, 10) == w.full[-2:] and ix.read(S + 1, 10) == b""
        assert ix.read_ranges([(0, 10), (co[3], 20), (5, 0)]) == [w.full[:10], w.full[co[3]:co[3] + 20], b""] and ix.read_ranges([]) == []
    damaged = bytearray(w.frame)
    damaged[w.payload_off[5] + 9] ^= 1
    with fr.FrameIndex(bytes(damaged)) as ix:                              # (create looks at no checksum)
        with pytest.raises(fr.BlockChecksumError):
            ix.read(co[5] + 1, 1)
        got = ix.read_ranges([(0, 10), (co[5], 3), (co[6], 3)], return_errors=True)
        assert got[0] == w.full[:10] and isinstance(got[1], fr.BlockChecksumError) and got[2] == w.full[co[6]:co[6] + 3]
    with pytest.raises(fr.IoError):
        fr.FrameIndex(w.frame[:-9])
    with pytest.raises(fr.DecompressionError) as e:
        fr.FrameIndex(FC.broken_frames()["offset 0 in the first sequence"])
    assert e.value.inner == "OffsetZero"
    # the device form, on torch tensors
    src = torch.from_numpy(np.frombuffer(w.frame, np.uint8).copy()).cuda()
    dst = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
    with fr.FrameIndex(src) as ix:
        assert ix.read(co[5] - 3, 10) == w.full[co[5] - 3:co[5] + 7]
        out_len, status = fr.read_ranges_device(ix, src, [(co[2] - 5, 30), (S - 1, 9)], dst, [101, 1003], stream=torch.cuda.current_stream().cuda_stream)
        assert (out_len, status) == ([30, 1], [0, 0])
        got = dst.cpu().numpy()
        assert got[101:131].tobytes() == w.full[co[2] - 5:co[2] + 25] and got[1003] == w.full[-1]
        assert (np.delete(got, list(range(101, 131)) + [1003]) == CANARY).all()
    # the command line
    path = tmp_path / "seven.lz4"
    path.write_bytes(w.frame)
    out = tmp_path / "piece"
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.check_call([sys.executable, "-m", "lz4_flex_amd.cli", str(path), "-o", str(out), "--range", "%d:%d" % (co[3] - 2, 70000)], env=env,
                          cwd=ROOT, stdout=subprocess.DEVNULL)
    assert out.read_bytes() == w.full[co[3] - 2:co[3] - 2 + 70000]
