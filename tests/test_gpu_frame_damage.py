"""GPU (-m gpu): every front end of the frame decoder on the damaged and truncated frames of tests/frame_damage_cases.py, about 700 per
base frame, against the oracle's FrameDecoder verdict O.frame_decompress(bytes, out_cap): the one-shot call, the streaming decoder (two
batch sizes), lz4flex_frame_decompress_many on host and on device memory and with the level-by-level Linked path, and
lz4flex_frame_index_create.  The oracle's verdicts are computed once per base frame and left alone.

The streaming decoder has no sink of its own: its verdict is the oracle's with room for everything (the short-sink cases are then five
more sound frames).  What it delivered before an error must be a prefix of what the ORACLE's reader had delivered when it stopped
(frame_damage_cases.delivered) -- for a frame that was only cut that is content[:content_off[k]]; a rewritten BlockInfo word or a flip
in an unchecked payload lets the reference itself hand out other bytes before it fails, so k alone does not bound it.

The decoders have no deviation from the oracle.  lz4flex_frame_index_create has the two rules of frame_damage_cases (reader_waits over the
cuts, reads_as_linked over one repaired header, each quoted from the public header there) and is judged on a checksum-free twin."""
import ctypes as C

import numpy as np
import pytest

import frame_damage_cases as D

pytestmark = pytest.mark.gpu
CANARY = 0xEE
FE_DECOMPRESSION, FE_IO, FE_UNSUPPORTED_BLOCKSIZE, FE_UNSUPPORTED_VERSION, FE_SKIPPABLE_FRAME, FE_CONTENT_LENGTH = 17, 18, 19, 20, 28, 30
FE_BLOCK_CHECKSUM, FE_CONTENT_CHECKSUM = 26, 27
E_HIP, E_UNSUPPORTED = 66, 68
ROOMY = D.CONTENT_LEN + D.SLACK
LINKED = [k for k in D.KEYS if k.startswith("lnk")]
INDEXED = [k for k in D.KEYS if k.startswith("ind-nosum")]


@pytest.fixture(scope="module")
def lib():
    from lz4_flex_amd import _lib
    l = _lib.load()
    assert l.lz4flex_device_count() >= 1
    return l


_held = {}


def _load(key):
    """(base, cases, the oracle's verdicts) of one base frame; one base frame is held at a time"""
    if _held.get("key") != key:
        _held.clear()
        cs = D.cases(key)
        _held.update(key=key, base=D.base(key), cases=cs, verdicts=[D.verdict(data, cap) for _, data, cap, _ in cs])
    return _held["base"], _held["cases"], _held["verdicts"]


def _each(items, check):
    """check(*item) for every item; all the cases that disagree are reported together"""
    bad = []
    for item in items:
        try:
            check(*item)
        except AssertionError as e:
            bad.append(str(e).split("\n")[0][:400])
    assert not bad, "%d of %d cases disagree with the oracle:\n%s" % (len(bad), len(items), "\n".join(bad[:60]))


def _detail(d):
    return int(d.expected), int(d.actual), int(d.inner)


def _check_failure(name, v, code, det):
    """status and every detail field the oracle fills for its code"""
    if code == -E_HIP:
        pytest.exit("a HIP error at %r: nothing more is run on this device" % name, returncode=3)
    assert code == -v.code, (name, code, det, v.code, v.detail)
    exp, act, inner = v.detail
    if v.code == FE_DECOMPRESSION:
        assert det[2] == inner, (name, det, v.detail)
        if inner == 1:
            assert det[:2] == (exp, act), (name, det, v.detail)
    elif v.code == FE_CONTENT_LENGTH:
        assert det[:2] == (exp, act), (name, det, v.detail)
    elif v.code in (FE_UNSUPPORTED_BLOCKSIZE, FE_UNSUPPORTED_VERSION, FE_SKIPPABLE_FRAME):
        assert det[0] == exp, (name, det, v.detail)


# ---- one-shot
@pytest.mark.parametrize("key", D.KEYS)
def test_one_shot(lib, key):
    from lz4_flex_amd import _lib
    _, cs, vs = _load(key)
    out = np.empty(ROOMY + 64, np.uint8)

    def check(case, v):
        name, data, cap, _ = case
        out[:] = CANARY
        used, d = C.c_size_t(0), _lib.ErrDetail()
        rc = lib.lz4flex_frame_decompress(data, len(data), C.c_void_p(out.ctypes.data), cap, C.byref(used), C.byref(d))
        assert (out[cap:] == CANARY).all(), name
        if v.code == 0:
            assert rc == v.out_len, (name, rc, _detail(d), v.out_len)
            assert out[:rc].tobytes() == v.output(), name
            assert used.value == v.consumed, (name, used.value, v.consumed)
        else:
            _check_failure(name, v, rc, _detail(d))
    _each(list(zip(cs, vs)), check)


# ---- streaming
def _stream(lib, data, batch_bytes):
    """read_to_end through the C decoder: (0 or the negative code, detail, the bytes delivered)"""
    from lz4_flex_amd import _lib
    src = C.create_string_buffer(data, max(len(data), 1))
    at = [0]

    def read(_user, buf, n):
        k = min(n, len(data) - at[0])
        C.memmove(buf, C.byref(src, at[0]), k)
        at[0] += k
        return k
    cb = _lib.READ_FN(read)
    h = lib.lz4flex_frame_decoder_new(cb, None)
    assert h
    try:
        if batch_bytes:
            assert lib.lz4flex_frame_decoder_set_batch_bytes(h, batch_bytes) == 0
        buf = C.create_string_buffer(1 << 20)
        got, d = [], _lib.ErrDetail()
        while True:
            r = lib.lz4flex_frame_decoder_read(h, C.cast(buf, C.c_void_p), len(buf), C.byref(d))
            if r <= 0:
                return int(r), _detail(d), b"".join(got)
            got.append(C.string_at(buf, r))
    finally:
        lib.lz4flex_frame_decoder_free(h)


@pytest.mark.parametrize("batch_bytes", [0, 65536])
@pytest.mark.parametrize("key", D.KEYS)
def test_streaming(lib, key, batch_bytes):
    b, cs, vs = _load(key)
    sparse = {"flip %d^5a" % o for o in range(0, len(b.frame), 509)}        # (the flips on every 509th byte are left to the other front ends)

    def check(case, v):
        name, data, cap, k = case
        if cap != ROOMY:
            v = D.verdict(data, ROOMY)
        rc, det, got = _stream(lib, data, batch_bytes)
        if v.code == 0:
            assert rc == 0 and got == v.output(), (name, rc, det, len(got), v.out_len)
        else:
            _check_failure(name, v, rc, det)
            before = D.delivered(data, ROOMY)
            assert got == before[:len(got)], (name, len(got), len(before))
            if D.family(name) == "cut":
                assert len(got) <= b.content_off[k], (name, len(got), k)
    _each([(c, v) for c, v in zip(cs, vs) if c[0] not in sparse], check)


# ---- many streams in one call
def _many(lib, items, mem, unaligned):
    """items: [(name, bytes, out_cap)].  Returns [(status, detail, bytes or None)]; asserts the call's return value, the canaries
    around every output region and the untouched frame buffer."""
    import torch
    from lz4_flex_amd import _lib
    n = len(items)
    in_off, in_len, out_off, out_cap, parts, at, oat = [], [], [], [], [], 0, 0
    for i, (_, data, cap) in enumerate(items):
        pad = 1 + i % 7 if unaligned else 0
        parts.append(b"\x5a" * pad); at += pad
        in_off.append(at); in_len.append(len(data)); parts.append(data); at += len(data)
        oat += 64
        oat += (5 - oat) % 16 if unaligned else 0
        out_off.append(oat); out_cap.append(cap); oat += cap
    oat += 64
    src = np.frombuffer(b"".join(parts) + b"\x5a", np.uint8)
    dst = np.full(oat, CANARY, np.uint8)
    a_io, a_il, a_oo, a_oc = (np.array(v, np.uint64) for v in (in_off, in_len, out_off, out_cap))
    out_len, status, detail = np.full(n, 77, np.uint64), np.full(n, 77, np.int32), (_lib.ErrDetail * n)()
    p = lambda a: C.c_void_p(a.ctypes.data)                                  # noqa: E731
    if mem == _lib.MEM_DEVICE:
        d_src, d_dst = torch.from_numpy(src.copy()).cuda(), torch.from_numpy(dst).cuda()
        rc = lib.lz4flex_frame_decompress_many(None, C.c_void_p(d_src.data_ptr()), p(a_io), p(a_il), n, C.c_void_p(d_dst.data_ptr()), p(a_oo), p(a_oc),
                                               p(out_len), p(status), detail, mem, None)
        got, back = d_dst.cpu().numpy(), d_src.cpu().numpy()
    else:
        keep = src.copy()
        rc = lib.lz4flex_frame_decompress_many(None, p(keep), p(a_io), p(a_il), n, p(dst), p(a_oo), p(a_oc), p(out_len), p(status), detail, mem, None)
        got, back = dst, keep
    if rc == -E_HIP:
        pytest.exit("a HIP error in lz4flex_frame_decompress_many: nothing more is run on this device", returncode=3)
    assert rc == 0, _lib.last_error()
    assert (back == src).all(), "the frame buffer was written to"
    outside = np.ones(oat, bool)
    for o, c in zip(out_off, out_cap):
        outside[o:o + c] = False
    assert (got[outside] == CANARY).all(), "bytes outside the streams' output regions were written"
    res = []
    for i in range(n):
        ok = status[i] == 0
        res.append((int(status[i]), _detail(detail[i]), got[out_off[i]:out_off[i] + int(out_len[i])].tobytes() if ok else None))
    return res


def _check_many(lib, key, mem, unaligned):
    """all cases of a base frame in ONE call (half a second on an MI355X)"""
    b, cs, vs = _load(key)
    sound = ("sound", b.frame, ROOMY)
    items = [(name, data, cap) for name, data, cap, _ in cs]
    mid = len(items) // 2 + 1
    items = [sound] + items[:mid - 1] + [sound] + items[mid - 1:] + [sound]     # the undamaged frame at 0, n / 2 and n - 1
    at = [i for i in range(len(items)) if i not in (0, mid, len(items) - 1)]
    res = _many(lib, items, mem, unaligned)
    for i in (0, mid, len(items) - 1):
        assert res[i][0] == 0 and res[i][2] == D.content(), ("the undamaged frame at", i, res[i][:2])

    def check(i, case, v):
        name = case[0]
        st, det, data = res[i]
        if v.code == 0:
            assert st == 0 and data == v.output(), (name, st, det, None if data is None else len(data), v.out_len)
        else:
            _check_failure(name, v, st, det)
    _each(list(zip(at, cs, vs)), check)


@pytest.mark.parametrize("key", D.KEYS)
def test_many_host(lib, key):
    from lz4_flex_amd import _lib
    _check_many(lib, key, _lib.MEM_HOST, False)


@pytest.mark.parametrize("key", D.KEYS)
def test_many_device(lib, key):
    """frames at unaligned offsets, 64 bytes of 0xEE behind every out_off + out_cap"""
    from lz4_flex_amd import _lib
    _check_many(lib, key, _lib.MEM_DEVICE, True)


@pytest.mark.parametrize("key", LINKED)
def test_many_level_by_level(lib, key):
    from lz4_flex_amd import _lib
    before = lib.lz4flex_get_tuning(None, b"decompress_level_chains")
    assert lib.lz4flex_set_tuning(None, b"decompress_level_chains", 1) == 0
    try:
        _check_many(lib, key, _lib.MEM_HOST, False)
    finally:
        assert lib.lz4flex_set_tuning(None, b"decompress_level_chains", before) == 0


# ---- the index
@pytest.mark.parametrize("mem", [0, 1], ids=["host", "device"])
@pytest.mark.parametrize("key", INDEXED)
def test_index_create(lib, key, mem):
    """the return value and detail of lz4flex_frame_index_create are the oracle's for the same bytes, but: no checksum is looked at -- the
    rule "a content that differs but is structurally sound succeeds": the oracle decides on frame_damage_cases.checksum_twin, the same
    frame with no checksum wrong, and create is held to that verdict exactly; and the two rules of frame_damage_cases, each an exact
    value too: a cut frame the reader would wait on is -FE_IO (reader_waits), a header that reads as Linked is -E_UNSUPPORTED
    (reads_as_linked).  Where an index is made its content_size is the oracle's output length.  Every index is freed."""
    import torch
    from lz4_flex_amd import _lib
    _, cs, vs = _load(key)

    def check(case, v):
        name, data, cap, _ = case
        if v.code in (FE_BLOCK_CHECKSUM, FE_CONTENT_CHECKSUM):
            v = D.verdict(D.checksum_twin(data), cap)
            assert v.code not in (FE_BLOCK_CHECKSUM, FE_CONTENT_CHECKSUM), name
        h, d = C.c_void_p(), _lib.ErrDetail()
        host = np.frombuffer(data + b"\0", np.uint8)
        if mem == _lib.MEM_DEVICE:
            dev = torch.from_numpy(host.copy()).cuda()
            rc = lib.lz4flex_frame_index_create(None, C.c_void_p(dev.data_ptr()), len(data), mem, C.byref(h), C.byref(d))
        else:
            rc = lib.lz4flex_frame_index_create(None, C.c_void_p(host.ctypes.data), len(data), mem, C.byref(h), C.byref(d))
        try:
            if D.reader_waits(name, v):
                assert rc == -FE_IO, (name, rc)
            elif D.reads_as_linked(name, data, v):
                assert rc == -E_UNSUPPORTED, (name, rc)
            elif v.code == 0:
                assert rc == 0, (name, rc, _detail(d))
                assert lib.lz4flex_frame_index_content_size(h) == v.out_len, (name, lib.lz4flex_frame_index_content_size(h), v.out_len)
            else:
                _check_failure(name, v, rc, _detail(d))
            assert bool(h) == (rc == 0), name
        finally:
            lib.lz4flex_frame_index_free(h)
    _each([(c, v) for c, v in zip(cs, vs) if D.family(c[0]) in ("flip", "cut", "header", "info", "block")], check)
