"""GPU tests of lz4flex_dict_train (lz4_dict_train.hip): the dictionary equals the scalar model's (tests/sim/dict_train_model.c) byte for
byte through MEM_DEVICE and MEM_HOST, with canaries around everything the call may write; then a trained dictionary end to end on the
device.  The status for 2^32 candidates or more is not run here -- it needs 4 GiB of samples; tests/test_dict_train_model.py covers that
path on the model alone."""
import ctypes as C

import numpy as np
import pytest

import dict_cases as D
import dict_train_model as M
import oracle_api as O

pytestmark = pytest.mark.gpu

MEMS = ["device", "host"]
CANARY = 0xC5
LEAD, TAIL = 64, 512
LENS = [0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 4096]
CAPS = [1, 7, 8, 63, 64, 65, 700, 32768, 65536]
SEGMENTS = [64, 512, 2048]


@pytest.fixture(scope="module")
def lib():
    from lz4_flex_amd import _lib
    lib = _lib.load()
    if lib.lz4flex_device_count() < 1:
        pytest.fail("GPU tests need a device: " + _lib.last_error())
    return lib


@pytest.fixture(scope="module")
def ctx(lib):
    c = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(c), -1) == 0
    yield c
    lib.lz4flex_ctx_destroy(c)


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _dev(a):
    import torch
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))


def call(lib, ctx, buf, offs, lens, cap, k, mem, big=False):
    """lz4flex_dict_train with canaries in front of and behind dict_out, around dict_len / status and (DEVICE) around work.  Checks them
    and that the input is unchanged; returns (dictionary bytes, status)."""
    from lz4_flex_amd import _lib
    n = len(offs)
    flags = _lib.MEM_BIG_BLOCKS if big else 0
    out = np.full(LEAD + cap + TAIL, CANARY, np.uint8)
    res = np.full(4, 0xA5A5A5A5, np.uint32)                  # canary, dict_len, status, canary
    if mem == "host":
        before = buf.copy()
        p = lambda a, at=0: C.c_void_p(a.ctypes.data + at) if a.size else None
        rc = lib.lz4flex_dict_train(ctx, p(buf), p(offs), p(lens), n, p(out, LEAD), cap, k, p(res, 4), p(res, 8), None, _lib.MEM_HOST | flags, None)
        assert rc == 0, (rc, _lib.last_error())
        assert (buf == before).all(), "the samples were written"
    else:
        import torch
        d_buf, d_offs, d_lens, d_out, d_res = _dev(buf), _dev(offs), _dev(lens), _dev(out), _dev(res)
        ws = int(lib.lz4flex_dict_train_work_size(n))
        work = torch.full((LEAD + ws + TAIL,), CANARY, dtype=torch.uint8, device=d_buf.device)
        stream = torch.cuda.current_stream(d_buf.device)
        p = lambda x, at=0: C.c_void_p(x.data_ptr() + at) if x.numel() else None
        rc = lib.lz4flex_dict_train(ctx, p(d_buf), p(d_offs), p(d_lens), n, p(d_out, LEAD), cap, k, p(d_res, 4), p(d_res, 8), p(work, LEAD),
                                    _lib.MEM_DEVICE | flags, C.c_void_p(stream.cuda_stream))
        assert rc == 0, (rc, _lib.last_error())
        stream.synchronize()
        assert bool((work[:LEAD] == CANARY).all()) and bool((work[LEAD + ws:] == CANARY).all()), "written outside work"
        assert (d_buf.cpu().numpy() == buf).all(), "the samples were written"
        out, res = d_out.cpu().numpy(), d_res.cpu().numpy().view(np.uint32)
    assert res[0] == 0xA5A5A5A5 and res[3] == 0xA5A5A5A5, "written around dict_len / status"
    dict_len, status = int(res[1]), int(res[2:3].view(np.int32)[0])
    assert dict_len <= cap
    assert (out[:LEAD] == CANARY).all(), "written in front of dict_out"
    assert (out[LEAD + dict_len:] == CANARY).all(), "written at or behind dict_out + dict_len"
    return out[LEAD:LEAD + dict_len].tobytes(), status


_want = {}


def want(key, buf, offs, lens, cap, k):
    """the model's answer, computed once per case and shared by the memory kinds"""
    if key not in _want:
        _want[key] = M.train_batch(buf, offs, lens, cap, k)
    return _want[key]


def check(lib, ctx, key, samples, cap, k, mem, packed=None, **kw):
    buf, offs, lens = packed if packed is not None else M.pack(samples)
    w = want((key, cap, k), buf, offs, lens, cap, k)
    got = call(lib, ctx, buf, offs, lens, cap, k, mem, **kw)
    assert got == w, "%s cap=%d k=%d %s: %d bytes, the model %d; first difference at %s" % (
        key, cap, k, mem, len(got[0]), len(w[0]), next((j for j, (x, y) in enumerate(zip(got[0], w[0])) if x != y), "the end"))
    return got[0]


def cut(kind, length, count, phase=0):
    flat = D.stream(kind, length * count, phase)
    return [flat[j * length:(j + 1) * length] for j in range(count)]


# ---- bytes equal the model's -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("kind", D.KINDS)
def test_lengths_caps_segments(lib, ctx, kind, mem):
    """six samples of every length x every capacity x every segment; zeros put every count on one counter and every flag but a sample's
    first to 0"""
    for length in LENS:
        samples = cut(kind, length, 6)
        for cap in CAPS:
            for k in SEGMENTS:
                check(lib, ctx, ("six", kind, length), samples, cap, k, mem)


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_batch_sizes(lib, ctx, n, mem):
    for kind in ("json", "log"):
        check(lib, ctx, ("n", kind, n), cut(kind, 300, n), 32768, 512, mem)
        check(lib, ctx, ("n", kind, n), cut(kind, 300, n), 1000, 64, mem)           # a capacity that is no multiple of the segment


@pytest.mark.parametrize("mem", MEMS)
def test_every_other_sample_too_short(lib, ctx, mem):
    full = cut("text", 700, 40)
    samples = [s if j % 2 == 0 else s[:(0, 3, 7, 1)[(j // 2) % 4]] for j, s in enumerate(full)]
    d = check(lib, ctx, "holes", samples, 4096, 256, mem)
    assert len(d) == 4096
    check(lib, ctx, "short", [b"abc", b"", b"1234567"], 32768, 512, mem)
    assert check(lib, ctx, "eight", [b"12345678"], 32768, 512, mem) == b"12345678"
    assert check(lib, ctx, "eight in the middle", [b"abc", b"12345678", b""], 32768, 0, mem) == b"12345678"


@pytest.mark.parametrize("mem", MEMS)
def test_known_answers(lib, ctx, mem):
    A, B = rnd(512, 1), rnd(512, 2)
    text = D.stream("text", 300, 0)
    assert check(lib, ctx, "tie", [A, B, A, B], 32768, 512, mem) == B + A            # a wrong tie-break gives A + B
    assert check(lib, ctx, "tie", [A, B, A, B], 700, 512, mem) == B[:188] + A        # the clipped last segment lands in front
    assert check(lib, ctx, "tie", [A, B, A, B], 32768, 0, mem) == B + A              # segment 0 is 512
    assert check(lib, ctx, "small cap", [text], 100, 512, mem) == text[:100]
    assert check(lib, ctx, "zeros", [bytes(4096)] * 4, 32768, 512, mem) == bytes(512)
    assert check(lib, ctx, "tie", [A, B, A, B], 32768, 512, mem, big=True) == B + A  # LZ4FLEX_MEM_BIG_BLOCKS changes nothing


@pytest.mark.parametrize("mem", MEMS)
def test_early_stop_leaves_the_output_alone(lib, ctx, mem):
    """1 000 copies of one sample: one segment, then E steps in a row without a winner end the run; the 120-odd steps behind that
    write nothing (call() checks the bytes behind the 300)"""
    text = D.stream("text", 300, 0)
    assert check(lib, ctx, "copies", [text] * 1000, 32768, 512, mem) == text


@pytest.mark.parametrize("mem", MEMS)
def test_regions_tiles_and_a_segment_across_a_region_boundary(lib, ctx, mem):
    """E = 4 regions of 5 569 candidates (22 273 in all: no multiple of E), three score tiles per region with a partial last one, one
    sample that spans all regions and several workgroups; a pattern that 40 small samples repeat lies across the first boundary, so the
    segment that wins region 0 starts in it and ends in region 1"""
    hot = rnd(64, 5)
    long = bytearray(rnd(20000, 6))
    long[5549:5549 + 64] = hot
    samples = [bytes(long)] + [hot] * 40
    buf, offs, lens = M.pack(samples)
    d, st, picks = M.train_batch(buf, offs, lens, 256, 64, with_picks=True)
    total, E = 19993 + 40 * 57, 4
    R = -(-total // E)
    assert total % E and total // (4 * 64) >= E and R == 5569
    assert (0, 5549, 64) in picks and 5549 < R < 5549 + 64
    assert check(lib, ctx, "boundary", samples, 256, 64, mem) == d
    for cap, k in ((1024, 64), (2048, 200), (8192, 512), (65536, 2048)):            # E = 16, 10, 9, 2
        check(lib, ctx, "boundary", samples, cap, k, mem)


@pytest.mark.parametrize("mem", MEMS)
def test_a_long_sample_among_short_ones(lib, ctx, mem):
    small = cut("json", 100, 100, phase=300000)
    samples = small[:50] + [D.stream("json", 200000, 0)] + small[50:]
    for cap, k in ((32768, 512), (65536, 2048), (3000, 64)):
        check(lib, ctx, "long", samples, cap, k, mem)


@pytest.mark.parametrize("mem", MEMS)
def test_thousands_of_empty_samples_between_long_ones(lib, ctx, mem):
    """a score tile whose window spans 4 096 sample indices or more cannot tell samples apart by their 12-bit tags: it limits every
    look-back by the position in the sample instead.  Text repeats, so a look-back that crossed into the sample in front would find
    hashes there"""
    text = D.stream("text", 12000, 0)
    samples = [text[:3000]] + [b""] * 4500 + [text[:3000]] + [b"x"] * 4500 + [text[3000:9000]] + [b"1234567"] * 5000 + [text[:6000]]
    for cap, k in ((4096, 512), (65536, 2048), (1024, 64)):
        check(lib, ctx, "sparse", samples, cap, k, mem)


@pytest.mark.parametrize("mem", MEMS)
def test_odd_offsets_overlap_and_descending_order(lib, ctx, mem):
    flat = np.frombuffer(D.stream("log", 50001, 0), np.uint8)
    offs = np.array([40001, 30003, 30001, 20001, 20001, 9, 1, 49999], np.uint64)          # odd, descending, two equal, overlapping
    lens = np.array([9000, 10500, 300, 15000, 8, 30000, 4099, 2], np.uint32)
    assert all(int(o) + int(ln) <= flat.size for o, ln in zip(offs, lens))
    for cap, k in ((32768, 512), (700, 100)):
        check(lib, ctx, "overlap", None, cap, k, mem, packed=(flat, offs, lens))


def test_nothing_to_do_on_the_device(lib, ctx):
    """n == 0 and dict_cap == 0: the two words are written by a kernel"""
    A = rnd(512, 1)
    empty = (np.zeros(1, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    assert call(lib, ctx, *empty, 32768, 512, "device") == (b"", 0)
    assert call(lib, ctx, *M.pack([A, A]), 0, 512, "device") == (b"", 0)


def test_two_calls_back_to_back_share_the_work(lib, ctx):
    """the DEVICE entry twice on one stream with different samples and the same `work`, no synchronisation in between"""
    import torch
    from lz4_flex_amd import _lib
    batches = [M.pack(cut("log", 4096, 64)), M.pack(cut("json", 1000, 300))]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    work = torch.empty(int(lib.lz4flex_dict_train_work_size(300)), dtype=torch.uint8, device=dev)
    keep, outs = [], []
    p = lambda x: C.c_void_p(x.data_ptr())
    for buf, offs, lens in batches:
        t = [_dev(buf), _dev(offs), _dev(lens), torch.zeros(32768, dtype=torch.uint8, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)]
        keep.append(t)
    for (buf, offs, lens), t in zip(batches, keep):
        rc = lib.lz4flex_dict_train(ctx, p(t[0]), p(t[1]), p(t[2]), len(offs), p(t[3]), 32768, 512, p(t[4][0:1]), p(t[4][1:2]), p(work),
                                    _lib.MEM_DEVICE, C.c_void_p(stream.cuda_stream))
        assert rc == 0
    stream.synchronize()
    for (buf, offs, lens), t in zip(batches, keep):
        n, st = (int(v) for v in t[4].cpu())
        outs.append(t[3].cpu().numpy()[:n].tobytes())
        assert (outs[-1], st) == M.train_batch(buf, offs, lens, 32768, 512)
    assert outs[0] != outs[1] and len(outs[0]) == 32768


# ---- end to end on the device ------------------------------------------------------------------------------------------------------
def test_trained_dictionary_end_to_end_on_the_device(lib):
    """1 024 records of 4 KiB (log, JSON, text) train a dictionary on the device; 96 records that are not among them go through the
    shared-dictionary and the dictionary-set calls with it and come back exactly, smaller than without a dictionary"""
    import torch
    from lz4_flex_amd import block
    dev = torch.device("cuda", 0)
    samples = cut("log", 4096, 512) + cut("json", 4096, 256) + cut("text", 4096, 256)
    unseen = [D.block(kind, 4096, salt) for kind in ("log", "json", "text") for salt in range(32)]
    buf, offs, lens = M.pack(samples)
    dictionary, dict_len = block.train_dictionary_device(_dev(buf), _dev(offs), _dev(lens))
    assert int(dict_len) == 32768
    trained = dictionary[:int(dict_len)]
    host = trained.cpu().numpy().tobytes()
    assert (host, 0) == M.train_batch(buf, offs, lens, 32768, 512)
    assert block.train_dictionary(samples) == host and block.train_dictionary_batch(buf, offs, lens) == host

    ubuf, uoffs, ulens = M.pack(unseen)
    src, d_off, d_len = _dev(ubuf), _dev(uoffs), _dev(ulens)
    comp, c_off, c_len, st = block.compress_blocks_with_shared_dict_device(src, d_off, d_len, trained)
    assert bool((st == 0).all())
    back, b_off, b_len, st = block.decompress_blocks_with_shared_dict_device(comp, c_off, c_len, trained)
    assert bool((st == 0).all())
    back, b_off, b_len = back.cpu().numpy(), b_off.cpu().numpy(), b_len.cpu().numpy()
    for j, u in enumerate(unseen):
        assert back[int(b_off[j]):int(b_off[j]) + int(b_len[j])].tobytes() == u, j
    comp_h, c_off_h, c_len_h = comp.cpu().numpy(), c_off.cpu().numpy(), c_len.cpu().numpy()
    for j in (0, 31, 32, 63, 64, 95):
        blk = comp_h[int(c_off_h[j]):int(c_off_h[j]) + int(c_len_h[j])].tobytes()
        assert O.decompress(blk, 4096, dict_data=host) == ("ok", unseen[j]), j

    caps = np.array([O.max_out(len(u)) for u in unseen], np.uint32)
    slots = np.concatenate([[0], np.cumsum(caps[:-1], dtype=np.uint64)]).astype(np.uint64)
    plain = np.zeros(int(caps.sum()) + 64, np.uint8)
    plain_len, st = block.compress_batch(ubuf, uoffs, ulens, plain, slots, caps)
    assert (st == 0).all()
    print("96 unseen records of 4 KiB: %d bytes with the trained dictionary, %d without" % (int(c_len.sum()), int(plain_len.sum())))
    assert int(c_len.sum()) < int(plain_len.sum())

    with block.DictSet([host]) as ds:
        ids = torch.zeros(len(unseen), dtype=torch.int32, device=dev)
        comp2, c_off2, c_len2, st = block.compress_blocks_with_dict_set_device(src, d_off, d_len, ids, ds)
        assert bool((st == 0).all()) and int(c_len2.sum()) < int(plain_len.sum())
        back2, b_off2, b_len2, st = block.decompress_blocks_with_dict_set_device(comp2, c_off2, c_len2, ids, ds)
        assert bool((st == 0).all())
        torch.cuda.synchronize(dev)
        back2, b_off2, b_len2 = back2.cpu().numpy(), b_off2.cpu().numpy(), b_len2.cpu().numpy()
        for j, u in enumerate(unseen):
            assert back2[int(b_off2[j]):int(b_off2[j]) + int(b_len2[j])].tobytes() == u, j
