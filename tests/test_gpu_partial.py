"""GPU (-m gpu): lz4flex_decompress_batch_partial -- the first target[i] bytes of every block, by the sequence decoder's partial form
(lz4_decompress_seq.hip) and by the reference-order form behind it (lz4_decompress.hip lz4_decompress_form_kernel<NoDict, true>).

Checker: tests/partial_model.py (the entry's contract in Python, pinned to the oracle by tests/test_partial_model.py) for status, out_len
and bytes; for valid blocks also the oracle's own bytes, cut at the target.  Every sink is exactly `target` bytes between canaries: a
byte stored at or behind out_off + target, or in front of out_off, fails the test.  The input buffer is compared with its copy."""
import ctypes as C

import numpy as np
import pytest

import corpus
import oracle_api as O
import partial_model as M
import seq_blocks

pytestmark = pytest.mark.gpu
REDO = 0x7F000001
CANARY = 64
FILL = 0xA5


@pytest.fixture(scope="module")
def env():
    import torch
    from lz4_flex_amd import _lib
    lib = _lib.load()
    assert lib.lz4flex_device_count() >= 1, _lib.last_error()
    return lib, _lib, torch


def _ctx(lib, **tuning):
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
    for k, v in tuning.items():
        assert lib.lz4flex_set_tuning(ctx, k.encode(), v) == 0, k
    return ctx


class Batch:
    """entries: (name, block, target); want: the model's (status, bytes) per entry.  Sink i: CANARY bytes of FILL, target bytes, CANARY
    bytes of FILL, at an out_off that is no multiple of 16; the blocks lie back to back from byte 3 of the input buffer."""

    def __init__(self, entries, want):
        self.entries, self.want, self.n = entries, want, len(entries)
        comps = [e[1] for e in entries]
        self.in_len = np.array([len(c) for c in comps], dtype=np.uint32)
        self.in_off = (np.concatenate([[0], np.cumsum(self.in_len[:-1], dtype=np.uint64)]) + 3).astype(np.uint64)
        self.inb = np.frombuffer(bytes(3) + b"".join(comps) + bytes(64), dtype=np.uint8).copy()
        self.target = np.array([e[2] for e in entries], dtype=np.uint32)
        off, o = [], 0
        for e in entries:
            o += CANARY
            if o % 16 == 0:
                o += 5
            off.append(o)
            o += e[2] + CANARY
        self.out_off = np.array(off, dtype=np.uint64)
        self.size = o + 64

    def sub(self, idx):
        return Batch([self.entries[i] for i in idx], [self.want[i] for i in idx])

    def run(self, env, ctx, mem, plain=False):
        """the partial entry (plain: lz4flex_decompress_batch with the targets as capacities): (out, out_len, status)"""
        lib, L, torch = env
        n = self.n
        out = np.full(self.size, FILL, dtype=np.uint8)
        arrays = dict(inb=self.inb.copy(), in_off=self.in_off, in_len=self.in_len, out=out, out_off=self.out_off, target=self.target,
                      out_len=np.full(n, 0xDEADBEEF, dtype=np.uint32), status=np.full(n, -1, dtype=np.int32))
        host = (mem & 0xFF) == L.MEM_HOST
        if host:
            keep, sp = arrays, None
            addr = {k: v.ctypes.data for k, v in arrays.items()}
        else:
            dev = torch.device("cuda", 0)
            keep = {k: torch.from_numpy(v.view(np.uint8).reshape(-1)).to(dev) for k, v in arrays.items()}
            addr = {k: v.data_ptr() for k, v in keep.items()}
            sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        p = {k: C.c_void_p(v) for k, v in addr.items()}
        if plain:
            rc = lib.lz4flex_decompress_batch(ctx, p["inb"], p["in_off"], p["in_len"], n, p["out"], p["out_off"], p["target"], p["out_len"],
                                              p["status"], None, mem, sp)
        else:
            rc = lib.lz4flex_decompress_batch_partial(ctx, p["inb"], p["in_off"], p["in_len"], n, p["out"], p["out_off"], p["target"],
                                                      p["out_len"], p["status"], mem, sp)
        assert rc == 0, (rc, L.last_error())
        if not host:
            torch.cuda.synchronize()
            for k in ("inb", "out", "out_len", "status"):
                arrays[k].view(np.uint8).reshape(-1)[:] = keep[k].cpu().numpy()
        assert np.array_equal(arrays["inb"], self.inb), "the input buffer was written"
        return out, arrays["out_len"], arrays["status"]

    def check(self, res, what, marked_ok=False):
        """status and out_len are the model's, the first out_len bytes of a sink too, and every byte outside the sinks is untouched (what
        a sink holds behind out_len, or after an error, is not specified).  marked_ok ("decompress_second_pass" 0): a block may instead
        be left marked with out_len 0.  Returns the marked blocks."""
        out, out_len, status = res
        exp = np.full(self.size, FILL, dtype=np.uint8)
        care = np.ones(self.size, dtype=bool)
        marked = []
        for i in range(self.n):
            name, (wst, wbytes) = self.entries[i][0], self.want[i]
            st, ol, o, t = int(status[i]), int(out_len[i]), int(self.out_off[i]), int(self.target[i])
            care[o:o + t] = False
            if marked_ok and st == REDO:
                assert ol == 0, (what, name, t)
                marked.append(i)
                continue
            assert (st, ol) == (wst, len(wbytes)), (what, name, t, hex(st), ol, wst, len(wbytes))
            if st == 0:
                exp[o:o + ol] = np.frombuffer(wbytes, dtype=np.uint8)
                care[o:o + ol] = True
        bad = np.nonzero((out != exp) & care)[0]
        if len(bad):
            b = int(bad[0])
            i = max(int(np.searchsorted(self.out_off, b, side="right")) - 1, 0)
            raise AssertionError("%s: %d wrong bytes, first at %d = sink %d (%s, target %d) + %d" %
                                 (what, len(bad), b, i, self.entries[i][0], int(self.target[i]), b - int(self.out_off[i])))
        return marked


MODES = [("device", 1), ("device", 0), ("host", 1), ("host", 0)]


def _mem(env, where, big=False):
    L = env[1]
    return (L.MEM_DEVICE if where == "device" else L.MEM_HOST) | (L.MEM_BIG_BLOCKS if big else 0)


# ---------------------------------------------------------------- 1. blocks written for the partial form's paths
_hand = {}


def hand_written():
    """the valid blocks of partial_model.writer_cases at each of their targets (checked against the oracle's bytes too) and the damaged
    ones of corrupted_cases: one Batch"""
    if not _hand:
        entries, want, valid = [], [], []
        for name, c, plain, targets in M.writer_cases():
            st, got = O.decompress(c, len(plain) + 64)
            for t in targets:
                w = M.partial(c, t)
                if st == "ok":
                    assert w == (0, got[:t]), (name, t)               # the oracle's bytes, cut at the target
                entries.append((name, c, t))
                want.append(w)
                valid.append(st == "ok")
        for name, c, targets in M.corrupted_cases():
            for t in targets:
                entries.append((name, c, t))
                want.append(M.partial(c, t))
                valid.append(False)
        _hand.update(batch=Batch(entries, want), valid=valid)
    return _hand["batch"], _hand["valid"]


@pytest.mark.parametrize("where,partial", MODES)
def test_hand_written_cut_points(env, where, partial):
    lib = env[0]
    batch, _ = hand_written()
    assert batch.n > 600 and {w[0] for w in batch.want} == {0, 2, 3, 4, 5}
    ctx = _ctx(lib, decompress_partial=partial)
    try:
        batch.check(batch.run(env, ctx, _mem(env, where)), "%s, decompress_partial %d" % (where, partial))
    finally:
        lib.lz4flex_ctx_destroy(ctx)


@pytest.mark.parametrize("where", ["device", "host"])
def test_batch_sizes_and_variant_1(env, where):
    """1 block, 65 blocks (two workgroups of the reference-order kernel and a ragged one), taken from the middle of the set; and
    "decompress_variant" 1, which selects the reference's order as "decompress_partial" 0 does"""
    lib = env[0]
    batch, _ = hand_written()
    ctx, ref = _ctx(lib), _ctx(lib, decompress_variant=1)
    try:
        for idx in ([137], list(range(100, 165)), list(range(batch.n - 65, batch.n))):
            b = batch.sub(idx)
            b.check(b.run(env, ctx, _mem(env, where)), "%s, %d blocks" % (where, b.n))
            b.check(b.run(env, ref, _mem(env, where)), "%s, %d blocks, decompress_variant 1" % (where, b.n))
    finally:
        lib.lz4flex_ctx_destroy(ctx)
        lib.lz4flex_ctx_destroy(ref)


# ---------------------------------------------------------------- 2. the generated sets
_gen = {}


def generated():
    """(name, block, capacity, Profile) of every block of seq_blocks.blocks() and corpus.adversarial_blocks(): one walk per block gives
    the model's result at every target (Profile.at == partial: tests/test_partial_model.py)"""
    if not _gen:
        rows = [(name, c, len(p)) for name, c, p in seq_blocks.blocks()]
        rows += [("adversarial %d" % i, c, cap) for i, (c, cap) in enumerate(corpus.adversarial_blocks())]
        _gen["rows"] = [(name, c, cap, M.Profile(c)) for name, c, cap in rows]
    return _gen["rows"]


def generated_batch(pick):
    rows = generated()
    entries = [(name, c, pick(cap)) for name, c, cap, _ in rows]
    return Batch(entries, [prof.at(e[2]) for e, (_, _, _, prof) in zip(entries, rows)])


PICKS = {"0": lambda cap: 0, "1": lambda cap: 1, "cap//2": lambda cap: cap // 2, "cap": lambda cap: cap}


@pytest.mark.parametrize("pick", list(PICKS))
def test_generated_sets(env, pick):
    """the whole set in one call, at one target rule, in every mode"""
    lib = env[0]
    batch = generated_batch(PICKS[pick])
    assert batch.n > 1500
    for where, partial in MODES:
        ctx = _ctx(lib, decompress_partial=partial)
        try:
            batch.check(batch.run(env, ctx, _mem(env, where)), "target %s, %s, decompress_partial %d" % (pick, where, partial))
        finally:
            lib.lz4flex_ctx_destroy(ctx)


# ---------------------------------------------------------------- 3. a large block
@pytest.mark.parametrize("where", ["device", "host"])
def test_one_large_block(env, where):
    """1 MiB of JSON, the first 100 bytes, LZ4FLEX_MEM_BIG_BLOCKS (a hint: the results do not depend on it)"""
    lib = env[0]
    data = (O.fixture_plain("compression_66k_JSON") * 17)[:1 << 20]
    c = O.compress(data)
    ctx = _ctx(lib)
    try:
        for big in (True, False):
            b = Batch([("1 MiB of JSON", c, 100)], [(0, data[:100])])
            b.check(b.run(env, ctx, _mem(env, where, big)), "%s, big %s" % (where, big))
    finally:
        lib.lz4flex_ctx_destroy(ctx)


# ---------------------------------------------------------------- 4. the kernel, not the fallback
def test_the_sequence_decoder_decodes_what_it_decodes_in_full(env):
    """"decompress_second_pass" 0: a block the partial form hands back stays marked.  At no target may it mark a block that the plain
    sequence decoder ("decompress_variant" 13), given the whole block and its full size in the same run, does not mark; and the plain
    sequence decoder marks none of the valid hand-written blocks."""
    lib, L, _ = env
    hand, valid = hand_written()
    blocks = {}
    for (name, c, _t), ok in zip(hand.entries, valid):
        if ok:
            blocks.setdefault(c, name)
    rows = generated()
    for name, c, cap, prof in rows[:len(seq_blocks.blocks())]:
        assert prof.status == 0 and len(prof.out) == cap, name
        blocks.setdefault(c, name)
    full = Batch([(name, c, len(M.Profile(c).out)) for c, name in blocks.items()], [M.partial(c, M.FOREVER) for c in blocks])
    plain_ctx = _ctx(lib, decompress_variant=13, decompress_second_pass=0)
    ctx = _ctx(lib, decompress_second_pass=0)
    try:
        marked = full.check(full.run(env, plain_ctx, L.MEM_DEVICE, plain=True), "the plain sequence decoder", marked_ok=True)
        plain_marked = {full.entries[i][1] for i in marked}
        hand_blocks = {c for (_n, c, _t), ok in zip(hand.entries, valid) if ok}
        assert not (plain_marked & hand_blocks), sorted(blocks[c] for c in plain_marked & hand_blocks)
        n_seq = len(seq_blocks.blocks())
        runs = [("hand-written", hand.sub([i for i, ok in enumerate(valid) if ok]))]
        runs += [("seq_blocks, target " + pick, generated_batch(PICKS[pick]).sub(range(n_seq))) for pick in PICKS]
        for what, b in runs:
            got = b.check(b.run(env, ctx, L.MEM_DEVICE), what, marked_ok=True)
            extra = [(b.entries[i][0], b.entries[i][2]) for i in got if b.entries[i][1] not in plain_marked]
            assert not extra, (what, extra[:10])
    finally:
        lib.lz4flex_ctx_destroy(plain_ctx)
        lib.lz4flex_ctx_destroy(ctx)


def test_second_pass_off_leaves_errors_marked(env):
    """a block whose error lies in front of the stop is handed back: marked, out_len 0, with "decompress_second_pass" 0"""
    lib, L, _ = env
    hand, _ = hand_written()
    idx = [i for i, w in enumerate(hand.want) if w[0] != 0]
    assert len(idx) > 40
    b = hand.sub(idx)
    ctx = _ctx(lib, decompress_second_pass=0)
    try:
        _, out_len, status = b.run(env, ctx, L.MEM_DEVICE)
        assert all(int(s) == REDO for s in status) and not out_len.any()
    finally:
        lib.lz4flex_ctx_destroy(ctx)


# ---------------------------------------------------------------- 5. the Python layer
def test_python_layer(env):
    """block.decompress_batch_partial and block.decompress_blocks_partial_device give the ctypes calls' results on 65 blocks;
    block.decompress_partial gives the bytes or raises the model's error"""
    lib, L, torch = env
    from lz4_flex_amd import block
    hand, _ = hand_written()
    idx = []
    for code in (2, 3, 4, 5):                                 # six blocks of every error, the rest valid ones from all over the set
        idx += [i for i, w in enumerate(hand.want) if w[0] == code][:6]
    good = [i for i, w in enumerate(hand.want) if w[0] == 0]
    idx += good[::len(good) // (65 - len(idx)) + 1]
    idx += [i for i in good if i not in idx][:65 - len(idx)]
    b = hand.sub(sorted(idx))
    assert b.n == 65 and {w[0] for w in b.want} == {0, 2, 3, 4, 5}
    ref = b.run(env, None, L.MEM_HOST)
    b.check(ref, "ctypes")
    out = np.full(b.size, FILL, dtype=np.uint8)
    out_len, status = block.decompress_batch_partial(b.inb, b.in_off, b.in_len, out, b.out_off, b.target)
    b.check((out, out_len, status), "decompress_batch_partial")
    assert np.array_equal(out_len, ref[1]) and np.array_equal(status, ref[2])
    dev = torch.device("cuda", 0)
    d_out, d_off, d_len, d_st = block.decompress_blocks_partial_device(torch.from_numpy(b.inb).to(dev), torch.from_numpy(b.in_off.astype(np.int64)),
                                                                       torch.from_numpy(b.in_len.astype(np.int64)),
                                                                       torch.from_numpy(b.target.astype(np.int64)))
    torch.cuda.synchronize()
    packed = d_out.cpu().numpy()
    off = d_off.cpu().numpy()
    assert packed.size == int(b.target.sum()) and np.array_equal(off, np.cumsum(b.target.astype(np.int64)) - b.target)
    assert np.array_equal(d_len.cpu().numpy().astype(np.uint32), ref[1]) and np.array_equal(d_st.cpu().numpy(), ref[2])
    errors = {2: block.LiteralOutOfBounds, 3: block.ExpectedAnotherByte, 4: block.OffsetZero, 5: block.OffsetOutOfBounds}
    raised = set()
    for i, ((name, c, t), (st, want)) in enumerate(zip(b.entries, b.want)):
        if st == 0:
            assert bytes(packed[int(off[i]):int(off[i]) + len(want)]) == want, name
            assert block.decompress_partial(c, t) == want, (name, t)
        else:
            with pytest.raises(errors[st]):
                block.decompress_partial(c, t)
            raised.add(st)
    assert raised == {2, 3, 4, 5}, raised
