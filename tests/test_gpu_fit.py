"""GPU tests of the fit batches (lz4flex_fit_batch, lz4flex_compress_batch_fit, lz4_fit.hip): the kernels equal tests/fit_model.py byte for
byte (out, out_len, in_used, status) on blocks that sit on the kernel's edges (tests/fit_cases.py), in both passes ("fit_serial" 0 / 1),
HOST and DEVICE; nothing outside [out_off, out_off + out_len) is written; damaged blocks give the reference's error in front of the cut
and go unseen behind it; compress_batch_fit is the model applied to compress_batch's bytes in every compress mode, and decodes."""
import ctypes as C

import numpy as np
import pytest

import fit_cases as K
import fit_model as F
import oracle_api as O

pytestmark = pytest.mark.gpu

GUARD, FILL = 32, 0xC5
FIRST_PASS = 2            # run_fit's `serial`: the hook "debug_fit_first_pass" instead of "fit_serial"
CANARY = 0x5A5A5A5A


@pytest.fixture(scope="module")
def lib():
    from lz4_flex_amd import _lib
    lib = _lib.load()
    if lib.lz4flex_device_count() < 1:
        pytest.fail("GPU tests need a device: " + _lib.last_error())
    return lib


@pytest.fixture
def ctx(lib):
    c = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(c), -1) == 0
    yield c
    lib.lz4flex_ctx_destroy(c)


def pack(parts, gap):
    offs, at = [], 1
    for p in parts:
        offs.append(at)
        at += len(p) + gap
    buf = np.full(at + 16, 0x77, np.uint8)
    for o, p in zip(offs, parts):
        buf[o:o + len(p)] = np.frombuffer(p, np.uint8)
    return buf, offs


def _dev(a):
    import torch
    v = a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a
    return torch.from_numpy(np.array(v)).to(torch.device("cuda", 0))


def run_fit(lib, ctx, pairs, items, mode, serial, extra=3):
    """pairs: [(block, source)], items: [(pair index, cap)].  Every item through lz4flex_fit_batch; returns [(out, in_used, status)] and
    checks that nothing but [out_off, out_off + out_len) of the output buffer and the n results was written."""
    from lz4_flex_amd import _lib
    assert lib.lz4flex_set_tuning(ctx, b"fit_serial", 1 if serial == 1 else 0) == 0
    assert lib.lz4flex_set_tuning(ctx, b"debug_fit_first_pass", 1 if serial == FIRST_PASS else 0) == 0
    blk_buf, blk_at = pack([p[0] for p in pairs], 3)
    src_buf, src_at = pack([p[1] for p in pairs], 5)
    n = len(items)
    blk_off = np.array([blk_at[i] for i, _ in items], np.uint64)
    blk_len = np.array([len(pairs[i][0]) for i, _ in items], np.uint32)
    src_off = np.array([src_at[i] for i, _ in items], np.uint64)
    src_len = np.array([len(pairs[i][1]) for i, _ in items], np.uint32)
    out_cap = np.array([cap for _, cap in items], np.uint32)
    out_off = np.zeros(n, np.uint64)
    at = 0
    for j, (_, cap) in enumerate(items):
        out_off[j] = at + GUARD + j % 5                       # (slots of every alignment)
        at += GUARD + j % 5 + cap
    out = np.full(at + GUARD, FILL, np.uint8)
    out_len, used, st = (np.full(n + extra, CANARY, dt) for dt in (np.uint32, np.uint32, np.int32))
    arrays = [blk_buf, blk_off, blk_len, src_buf, src_off, src_len, out, out_off, out_cap, out_len, used, st]
    if mode == "host":
        p = [C.c_void_p(a.ctypes.data) for a in arrays]
        rc = lib.lz4flex_fit_batch(ctx, *p[:6], n, *p[6:], _lib.MEM_HOST, None)
        assert rc == 0, _lib.last_error()
    else:
        import torch
        t = [_dev(a) for a in arrays]
        p = [C.c_void_p(x.data_ptr()) for x in t]
        stream = torch.cuda.current_stream(torch.device("cuda", 0))
        rc = lib.lz4flex_fit_batch(ctx, *p[:6], n, *p[6:], _lib.MEM_DEVICE | _lib.MEM_BIG_BLOCKS, C.c_void_p(stream.cuda_stream))
        assert rc == 0, _lib.last_error()
        stream.synchronize()
        out = t[6].cpu().numpy()
        out_len, used, st = t[9].cpu().numpy().view(np.uint32), t[10].cpu().numpy().view(np.uint32), t[11].cpu().numpy()
    assert (out_len[n:] == CANARY).all() and (used[n:] == CANARY).all() and (st[n:] == CANARY).all(), "results written past n"
    untouched = np.ones(out.size, bool)
    res = []
    for j in range(n):
        o, ln = int(out_off[j]), int(out_len[j])
        assert ln <= items[j][1], (j, ln, items[j][1])
        untouched[o:o + ln] = False
        res.append((out[o:o + ln].tobytes(), int(used[j]), int(st[j])))
    assert (out[untouched] == FILL).all(), "bytes outside [out_off, out_off + out_len) were written"
    return res


@pytest.fixture(scope="module")
def cases():
    """the blocks, the (block, cap) items and the model's answers, computed once"""
    shapes, small = K.shapes(), K.small_blocks()
    pairs = [(b, p) for _, b, p in shapes + small]
    items = [(i, cap) for i, (_, b, _) in enumerate(shapes) for cap in K.shape_caps(b)]
    items += [(len(shapes) + i, cap) for i in range(len(small)) for cap in range(0, 301)]
    want = [F.fit(pairs[i][0], pairs[i][1], cap) for i, cap in items]
    names = [(shapes + small)[i][0] for i, _ in items]
    return pairs, items, want, names


def compare(got, want, items, names):
    bad = [(names[j], items[j][1], g[1:], w[1:], len(g[0]), len(w[0])) for j, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("serial", [0, 1])
def test_kernel_equals_model(lib, ctx, cases, mode, serial):
    pairs, items, want, names = cases
    compare(run_fit(lib, ctx, pairs, items, mode, serial), want, items, names)


FIT_REDO = 0x7F000004


def test_the_wavefront_pass_finishes_every_valid_block(lib, ctx, cases):
    """the hook "debug_fit_first_pass": the wavefront pass alone -- it hands no valid block of the cases to the reference-order pass, and
    every damaged one"""
    pairs, items, want, names = cases
    compare(run_fit(lib, ctx, pairs, items, "device", FIRST_PASS), want, items, names)
    dmg = K.damaged()
    got = run_fit(lib, ctx, [(b, p) for _, b, p, _, _ in dmg], [(i, len(d[1]) - 1) for i, d in enumerate(dmg)], "device", FIRST_PASS)
    assert got == [(b"", 0, FIT_REDO)] * len(dmg)


def test_the_cases_take_every_path(cases):
    """what the shapes are for: cuts that are Clipped, cuts that are not at the last feasible k, blocks that fit, the one status of cap 0"""
    pairs, items, want, names = cases
    zero = [w for (i, cap), w, nm in zip(items, want, names) if nm == "zero_run" and 12 <= cap < len(pairs[i][0])]
    assert zero and all(st == 0 and used > 500 for _, used, st in zero)              # Clipped on a length run
    assert all(w == (b"", 0, F.E_OUTPUT_TOO_SMALL) for (i, cap), w in zip(items, want) if cap == 0)
    assert sum(1 for (i, cap), w in zip(items, want) if cap >= len(pairs[i][0]) and w[0] == pairs[i][0]) >= 2 * 18
    assert all(w[2] == 0 for (i, cap), w in zip(items, want) if cap > 0)


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("serial", [0, 1])
def test_damaged_blocks(lib, ctx, mode, serial):
    dmg = K.damaged()
    pairs = [(b, p) for _, b, p, _, _ in dmg]
    items, want = [], []
    for i, (name, block, plain, at, code) in enumerate(dmg):
        for cap in (at + 1, at + 2, len(block) - 1):          # in front of the cut: the reference's error, nothing written
            items.append((i, cap))
            want.append((b"", 0, code))
        for cap in (1, 7, at // 2, at - 1, at):              # behind it: not seen
            items.append((i, cap))
            w = F.fit(block, plain, cap)
            assert w[2] == 0 and O.decompress(w[0], max(w[1], 1)) == ("ok", plain[:w[1]])
            want.append(w)
        items.append((i, len(block)))                         # a block that fits is copied, not walked
        want.append((block, len(plain), 0))
    compare(run_fit(lib, ctx, pairs, items, mode, serial), want, items, [dmg[i][0] for i, _ in items])


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("serial", [0, 1])
def test_a_wrong_source_length_still_gives_a_valid_block(lib, ctx, mode, serial):
    """src_len is a promise that is not checked: with a wrong one the kernels still equal the model, inside cap and structurally valid"""
    shapes = [K.count_block(20, 5), K.grid_block(), K.zero_run_block(5000)]
    pairs, items = [], []
    for block, plain in shapes:
        for n in (0, 1, 7, len(plain) // 2):
            pairs.append((block, plain[:n]))
            items += [(len(pairs) - 1, cap) for cap in (1, 6, 20, len(block) // 2, len(block) - 1)]
    want = [F.fit(pairs[i][0], pairs[i][1], cap) for i, cap in items]
    for (i, cap), (out, used, st) in zip(items, want):
        assert st == 0 and len(out) <= cap and used <= len(pairs[i][1])
        assert O.decompress(out, 400000)[0] == "ok"
    compare(run_fit(lib, ctx, pairs, items, mode, serial), want, items, ["wrong_src_len"] * len(items))


# ---- composition: the encoder in front of the fit pass -------------------------------------------------------------------------------
BLOCK = 4096
MODES = [("fast", None), ("exact", None), ("high", 4)]


@pytest.fixture(scope="module")
def records():
    """64 blocks of 4 KiB: JSON, text, runs, noise"""
    import corpus
    m = O.manifest()["compression_66k_JSON"]
    st, json = O.decompress(O.golden_block("compression_66k_JSON"), m["plain_len"])
    assert st == "ok"
    text = (corpus.COMPRESSION_WORKS * 150)[:24 * BLOCK]
    data = json[:16 * BLOCK] + text + corpus.lcg_bytes(12 * BLOCK, 3, alphabet=6, run=9) + corpus.lcg_bytes(8 * BLOCK, 5, alphabet=64) + \
        bytes(2 * BLOCK) + corpus.lcg_bytes(2 * BLOCK, 11)
    assert len(data) == 64 * BLOCK
    return data


@pytest.fixture
def compress_mode():
    from lz4_flex_amd import block

    def choose(mode, depth):
        block.set_compress_mode(mode)
        if depth:
            block.set_compress_depth(depth)
    yield choose
    block.set_compress_mode("fast")
    block.set_compress_depth(16)


@pytest.mark.parametrize("mode,depth", MODES, ids=[m for m, _ in MODES])
def test_compress_batch_fit_is_the_model_of_compress_batch(lib, records, compress_mode, mode, depth):
    import torch
    from lz4_flex_amd import block
    compress_mode(mode, depth)
    max_out = block.get_maximum_output_size(BLOCK)
    caps = [64, 1024, 4096, max_out]
    src = np.frombuffer(records, np.uint8)
    in_off = np.array([BLOCK * (j // len(caps)) for j in range(64 * len(caps))], np.uint64)       # every block once per cap: ONE batch
    in_len = np.full(in_off.size, BLOCK, np.uint32)
    cap = np.array(caps * 64, np.uint32)
    n = in_off.size
    # lz4flex_compress_batch's bytes for the same batch under the same settings
    slots = np.arange(n, dtype=np.uint64) * max_out
    ref = np.zeros(n * max_out, np.uint8)
    ref_len, ref_st = block.compress_batch(src, in_off, in_len, ref, slots, np.full(n, max_out, np.uint32))
    assert (ref_st == 0).all()
    want = []
    for j in range(n):
        plain = records[int(in_off[j]):int(in_off[j]) + BLOCK]
        blk = ref[int(slots[j]):int(slots[j]) + int(ref_len[j])].tobytes()
        want.append(F.fit(blk, plain, int(cap[j])))
    assert any(len(w[0]) < int(ref_len[j]) for j, w in enumerate(want)) and all(w[2] == 0 for w in want)
    # HOST
    out_off = np.cumsum(cap, dtype=np.uint64) - cap
    out = np.full(int(cap.sum()), FILL, np.uint8)
    out_len, used, st = block.compress_batch_fit(src, in_off, in_len, out, out_off, cap)
    got = [(out[int(o):int(o) + int(ln)].tobytes(), int(u), int(s)) for o, ln, u, s in zip(out_off, out_len, used, st)]
    bad = [(j, int(cap[j]), g[1:], w[1:]) for j, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (mode, "host", len(bad), bad[:8])
    for j in range(n):
        assert (out[int(out_off[j]) + int(out_len[j]):int(out_off[j]) + int(cap[j])] == FILL).all(), j
    full = cap == max_out
    assert (used[full] == BLOCK).all() and (out_len[full] == ref_len[full]).all()
    # DEVICE, and every output decoded on the GPU
    dev = torch.device("cuda", 0)
    d_src = torch.from_numpy(np.array(src)).to(dev)
    d_out, d_off, d_len, d_used, d_st = block.compress_blocks_fit_device(d_src, torch.from_numpy(in_off.astype(np.int64)),
                                                                        torch.from_numpy(in_len.astype(np.int64)), torch.from_numpy(cap.astype(np.int64)))
    torch.cuda.synchronize()
    assert (d_off.cpu().numpy().astype(np.uint64) == out_off).all()
    h_out, h_len = d_out.cpu().numpy(), d_len.cpu().numpy().view(np.uint32)
    got = [(h_out[int(o):int(o) + int(ln)].tobytes(), int(u), int(s)) for o, ln, u, s in zip(out_off, h_len, d_used.cpu().numpy(), d_st.cpu().numpy())]
    bad = [(j, int(cap[j]), g[1:], w[1:]) for j, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (mode, "device", len(bad), bad[:8])
    dec = np.zeros(n * BLOCK, np.uint8)
    dec_off = np.arange(n, dtype=np.uint64) * BLOCK
    dec_len, dec_st, _ = block.decompress_batch(h_out, out_off, h_len, dec, dec_off, used)
    assert (dec_st == 0).all() and (dec_len == used).all()
    for j in range(n):
        assert dec[int(dec_off[j]):int(dec_off[j]) + int(used[j])].tobytes() == records[int(in_off[j]):int(in_off[j]) + int(used[j])], j


def test_a_scratch_slot_behind_scratch_cap_is_output_too_small(lib, records):
    """MEM_DEVICE: the slots are laid out on the device; a block whose slot ends behind scratch_cap gets OUTPUT_TOO_SMALL through the
    gated fit pass, the blocks in front of it are what they are with room for all"""
    import torch
    from lz4_flex_amd import block
    dev = torch.device("cuda", 0)
    n, room_for = 16, 10
    d_src = torch.from_numpy(np.frombuffer(records[:n * BLOCK], np.uint8).copy()).to(dev)
    in_off, in_len = torch.arange(n, dtype=torch.int64) * BLOCK, torch.full((n,), BLOCK, dtype=torch.int64)
    cap = torch.full((n,), 1024, dtype=torch.int64)
    slot = block.get_maximum_output_size(BLOCK)
    full = [t.cpu().numpy() for t in block.compress_blocks_fit_device(d_src, in_off, in_len, cap)]
    part = [t.cpu().numpy() for t in block.compress_blocks_fit_device(d_src, in_off, in_len, cap, scratch_cap=room_for * slot + slot - 1)]
    assert (full[4] == 0).all() and (full[2] > 0).all()
    assert (part[4][:room_for] == 0).all() and (part[4][room_for:] == F.E_OUTPUT_TOO_SMALL).all()
    assert (part[2][room_for:] == 0).all() and (part[3][room_for:] == 0).all()
    assert (part[2][:room_for] == full[2][:room_for]).all() and (part[3][:room_for] == full[3][:room_for]).all()
    for j in range(room_for):
        o, ln = int(full[1][j]), int(full[2][j])
        assert part[0][o:o + ln].tobytes() == full[0][o:o + ln].tobytes(), j


def test_python_forms(lib, records):
    """fit_batch, fit_blocks_device and the scalar compress_fit against the model"""
    import torch
    from lz4_flex_amd import block
    shapes = K.small_blocks() + [s for s in K.shapes() if s[0] in ("lit16", "count64", "zero_run")]
    blk_buf, blk_at = pack([b for _, b, _ in shapes], 0)
    src_buf, src_at = pack([p for _, _, p in shapes], 0)
    caps = [len(b) // 2 for _, b, _ in shapes]
    want = [F.fit(b, p, c) for (_, b, p), c in zip(shapes, caps)]
    blk_len, src_len = [len(b) for _, b, _ in shapes], [len(p) for _, _, p in shapes]
    out_off = np.cumsum(caps) - np.array(caps)
    out = np.zeros(sum(caps), np.uint8)
    out_len, used, st = block.fit_batch(blk_buf, blk_at, blk_len, src_buf, src_at, src_len, out, out_off, caps)
    assert [(out[int(o):int(o) + int(ln)].tobytes(), int(u), int(s)) for o, ln, u, s in zip(out_off, out_len, used, st)] == want
    dev = torch.device("cuda", 0)
    i64 = lambda a: torch.tensor(list(a), dtype=torch.int64)     # noqa: E731
    d_out, d_off, d_len, d_used, d_st = block.fit_blocks_device(torch.from_numpy(blk_buf).to(dev), i64(blk_at), i64(blk_len),
                                                                torch.from_numpy(src_buf).to(dev), i64(src_at), i64(src_len), i64(caps))
    torch.cuda.synchronize()
    h = d_out.cpu().numpy()
    assert [(h[int(o):int(o) + int(ln)].tobytes(), int(u), int(s))
            for o, ln, u, s in zip(d_off.cpu().numpy(), d_len.cpu().numpy(), d_used.cpu().numpy(), d_st.cpu().numpy())] == want
    # the scalar form: whatever fits a 4 KiB page of a 16 KiB record
    data = records[:4 * BLOCK]
    page, n_used = block.compress_fit(data, 4096)
    assert len(page) <= 4096 and 4096 < n_used < len(data)
    assert block.decompress(page, n_used) == data[:n_used]
    whole, n_all = block.compress_fit(data, block.get_maximum_output_size(len(data)))
    assert n_all == len(data) and whole == block.compress(data)
    with pytest.raises(block.CompressOutputTooSmall):
        block.compress_fit(data, 0)
