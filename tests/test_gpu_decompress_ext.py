"""GPU (-m gpu): lz4flex_decompress_batch_ex, the entry that decodes Linked frames, in the three modes in which a match may read bytes the
block did not write itself -- prefix (ext->out_pos), chained (LZ4FLEX_MEM_CHAINED, one chain or several: chain_prev) and dictionary --
called directly, with the shapes the frame layer never produces: prefixes of 0 ... 17 bytes, around the sequence decoder's KEEP / window
(1 280 / 3 584) and 64 KiB, a prefix of which only the last 64 KiB is reachable, blocks larger than 64 KiB behind a prefix, ragged chains.

Checker: the oracle's decompress_internal with a sink position (oracle_api.decompress_prefix): status, out_len (new bytes only), the
bytes, the OutputTooSmall {expected, actual} detail (absolute: it counts the prefix), the prefix untouched, nothing written behind
out_off + out_cap.  The blocks come from tests/ext_cases.py, whose meaning tests/test_decompress_ext_oracle.py pins on the CPU."""
import ctypes as C
import random

import numpy as np
import pytest

import ext_cases as X
import oracle_api as O
from lz4_writer import Writer

pytestmark = pytest.mark.gpu
REDO = 0x7F000001
INVALID_ARG = 64
CANARY = 256
FILL = 0xA5
ERR_CODES = {v: k for k, v in O.ERR_NAMES.items()}


@pytest.fixture(scope="module")
def env():
    import torch
    from lz4_flex_amd import _lib
    lib = _lib.load()
    assert lib.lz4flex_device_count() >= 1, _lib.last_error()
    return lib, _lib, torch


def _decoders(lib):
    """every configuration the library can be pinned to (lz4flex_get_tuning "decoder_config_<i>" = variant * 1000 + parameter)"""
    out, i = [], 0
    while True:
        v = lib.lz4flex_get_tuning(None, b"decoder_config_%d" % i)
        if v < 0:
            break
        out.append(divmod(v, 1000))
        i += 1
    assert {1, 4, 7, 8, 13} <= {v for v, _ in out}, out
    return out


def _ctx(lib, variant=0, par=0, **tuning):
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
    if variant:
        assert lib.lz4flex_set_tuning(ctx, b"decompress_variant", variant) == 0
    if variant == 1 and par:
        assert lib.lz4flex_set_tuning(ctx, b"decompress_lanes", par) == 0
    if variant == 4 and par:
        assert lib.lz4flex_set_tuning(ctx, b"decompress_blocks_per_wg", par) == 0
    for k, v in tuning.items():
        assert lib.lz4flex_set_tuning(ctx, k.encode(), v) == 0, k
    return ctx


# ---------------------------------------------------------------- a batch: layout, expected image, run, check
class Batch:
    """cases: (name, block, prefix, cap, dict or None[, expected]).  Every case gets a region of its own: the prefix, then FILL up to
    max(cap, prefix) + `slack` + CANARY.  `want` is the oracle's verdict, or ("InvalidArg",) for cap < len(prefix)."""

    def __init__(self, cases, slack=0, misalign=3, chain=None):
        self.cases = cases
        self.dont_care_from = None                    # (a chain behind an invalid block: what its later blocks do is not specified)
        n = len(cases)
        self.n = n
        comps = [c[1] for c in cases]
        self.in_len = np.array([len(c) for c in comps], dtype=np.uint32)
        self.in_off = (np.concatenate([[0], np.cumsum(self.in_len[:-1], dtype=np.uint64)]) + misalign).astype(np.uint64)
        self.inb = np.frombuffer(bytes(misalign) + b"".join(comps) + bytes(64), dtype=np.uint8).copy()
        self.cap = np.array([c[3] for c in cases], dtype=np.uint32)
        self.pos = np.array([len(c[2]) for c in cases], dtype=np.uint32)
        self.want = []
        for c in cases:
            if len(c) > 5:
                self.want.append(c[5])
            elif c[3] < len(c[2]):
                self.want.append(("InvalidArg",))
            else:
                self.want.append(O.decompress_prefix(c[1], c[2], c[3], dict_data=c[4]))
        if chain is None:
            sizes = [max(int(self.cap[i]), int(self.pos[i])) + slack + CANARY for i in range(n)]
            self.out_off = (np.concatenate([[0], np.cumsum(sizes[:-1], dtype=np.uint64)]) + misalign).astype(np.uint64)
            total = int(self.out_off[-1]) + sizes[-1] + 64
            self.init = np.full(total, FILL, dtype=np.uint8)
            for i, c in enumerate(cases):
                o = int(self.out_off[i])
                self.init[o:o + len(c[2])] = np.frombuffer(c[2], dtype=np.uint8)
            self.ends = [int(self.out_off[i]) + sizes[i] for i in range(n)]
        else:                                         # (one chain: every block shares the region, chain = the bytes before block 0)
            self.out_off = np.full(n, misalign, dtype=np.uint64)
            total = misalign + max(max(int(self.cap[i]), int(self.pos[i])) for i in range(n)) + slack + CANARY + 64
            self.init = np.full(total, FILL, dtype=np.uint8)
            self.init[misalign:misalign + len(chain)] = np.frombuffer(chain, dtype=np.uint8)
            self.ends = None
        dicts = [c[4] for c in cases]
        self.has_dict = any(d is not None for d in dicts)
        if self.has_dict:
            dl = [len(d or b"") for d in dicts]
            self.dict_len = np.array(dl, dtype=np.uint32)
            self.dict_off = (np.concatenate([[0], np.cumsum([k + 1 for k in dl[:-1]], dtype=np.uint64)]) + 1).astype(np.uint64)   # odd offsets
            self.dictb = np.frombuffer(b"\x00" + b"".join((d or b"") + b"\x00" for d in dicts) + bytes(64), dtype=np.uint8).copy()

    def expected(self, device):
        """the image the output buffer must have, and where it must have it"""
        exp = self.init.copy()
        care = np.ones(len(exp), dtype=bool)
        for i, w in enumerate(self.want):
            o, p, cap = int(self.out_off[i]), int(self.pos[i]), int(self.cap[i])
            if w[0] == "ok":
                exp[o + p:o + p + len(w[1])] = np.frombuffer(w[1], dtype=np.uint8)
                if device:
                    care[o + p + len(w[1]):o + cap] = False      # (wide stores may rewrite sink bytes behind the block's end)
            elif w[0] != "InvalidArg":
                care[o + p:o + cap] = False                      # a failed block may have written part of its sink
        if self.dont_care_from is not None:
            care[self.dont_care_from:] = False
        return exp, care

    def run(self, env, ctx, mem, flags=0, chain_prev=None, n_chains=0, n=None):
        lib, L, torch = env
        n = self.n if n is None else n
        out = self.init.copy()
        out_len = np.full(n, 0xDEADBEEF, dtype=np.uint32)
        status = np.full(n, -1, dtype=np.int32)
        detail = np.full((n, 2), 0xEE, dtype=np.uint64)
        ext = L.DecompressExt()
        arrays = dict(inb=self.inb, in_off=self.in_off, in_len=self.in_len, out=out, out_off=self.out_off, cap=self.cap,
                      pos=self.pos, out_len=out_len, status=status, detail=detail)
        if self.has_dict:
            arrays.update(dictb=self.dictb, dict_off=self.dict_off, dict_len=self.dict_len)
        if chain_prev is not None:
            arrays["chain_prev"] = np.ascontiguousarray(chain_prev, dtype=np.uint32)
        if mem == L.MEM_HOST:
            keep = arrays
            ptr = {k: C.c_void_p(v.ctypes.data) for k, v in arrays.items()}
            stream = None
        else:
            dev = torch.device("cuda", 0)
            keep = {k: torch.from_numpy(v.view(np.uint8).reshape(-1)).to(dev) for k, v in arrays.items()}
            ptr = {k: C.c_void_p(v.data_ptr()) for k, v in keep.items()}
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        ext.out_pos = ptr["pos"]
        if self.has_dict:
            ext.dict_base, ext.dict_off, ext.dict_len = ptr["dictb"], ptr["dict_off"], ptr["dict_len"]
        if chain_prev is not None:
            ext.chain_prev, ext.n_chains = ptr["chain_prev"], n_chains
        rc = lib.lz4flex_decompress_batch_ex(ctx, ptr["inb"], ptr["in_off"], ptr["in_len"], n, ptr["out"], ptr["out_off"], ptr["cap"],
                                             ptr["out_len"], ptr["status"], ptr["detail"], C.byref(ext), mem | flags, stream)
        assert rc == 0, (rc, L.last_error())
        if mem != L.MEM_HOST:
            torch.cuda.synchronize()
            for k in ("out", "out_len", "status", "detail"):
                arrays[k].view(np.uint8).reshape(-1)[:] = keep[k].cpu().numpy()
        return out, out_len, status, detail

    def check(self, res, device, what, second_pass=True, n=None):
        out, out_len, status, detail = res
        n = self.n if n is None else n
        for i in range(n):
            name, w = self.cases[i][0], self.want[i]
            st, ol = int(status[i]), int(out_len[i])
            if not second_pass and st == REDO:
                assert w[0] != "ok", "%s: %s: a valid block was left to the second pass" % (what, name)
                continue
            if w[0] == "ok":
                assert (st, ol) == (0, len(w[1])), (what, name, st, ol, len(w[1]))
            elif w[0] == "InvalidArg":
                assert (st, ol, int(detail[i][0]), int(detail[i][1])) == (INVALID_ARG, 0, 0, 0), (what, name, st, ol, detail[i])
            else:
                assert (st, ol) == (ERR_CODES[w[0]], 0), (what, name, st, ol, w)
                if w[0] == "OutputTooSmall":
                    assert (int(detail[i][0]), int(detail[i][1])) == tuple(w[1]), (what, name, detail[i], w[1])
        exp, care = self.expected(device)
        if not second_pass:
            for i in range(n):
                if int(status[i]) == REDO:
                    o = int(self.out_off[i])
                    care[o + int(self.pos[i]):o + int(self.cap[i])] = False
        lim = self.ends[n - 1] if self.ends is not None else len(out)
        bad = np.nonzero((out[:lim] != exp[:lim]) & care[:lim])[0]
        if len(bad):
            at = int(bad[0])
            i = int(np.searchsorted(self.out_off[:n], at, side="right")) - 1 if self.ends is not None else -1
            o = int(self.out_off[i]) if i >= 0 else 0
            where = "prefix" if at - o < int(self.pos[i]) else ("canary" if at - o >= max(int(self.cap[i]), int(self.pos[i])) else "sink")
            raise AssertionError("%s: %s: %d wrong bytes, the first at %d of its region (%s)" % (what, self.cases[i][0] if i >= 0 else "chain",
                                                                                           len(bad), at - o, where))


def _caps(name, c, prefix, new):
    """exact, 777 more, none (cap == out_pos), 1 and 40 short (never below the prefix), the block cut short"""
    p = len(prefix)
    out = []
    if new is None:
        return [(name, c, prefix, p + 100, None)]
    exact = p + len(new)
    for tag, cap in (("exact", exact), ("+777", exact + 777), ("no room", p), ("1 short", exact - 1), ("40 short", exact - 40)):
        if cap >= p and (tag == "exact" or cap != exact):
            out.append(("%s, cap %s" % (name, tag), c, prefix, cap, None))
    if len(c) > 3:
        out.append(("%s, cut" % name, c[:-3], prefix, exact, None))
    return out


@pytest.fixture(scope="module")
def prefix_cases(env):
    """group A: writer blocks behind every prefix length, a 1 MiB block behind 64 KiB, the oracle's Linked-frame blocks at their true
    positions (64 KiB and 256 KiB blocks), throughput-encoder blocks written with LZ4FLEX_BLOCK_HISTORY(h) behind those h bytes"""
    lib, L, torch = env
    from lz4_flex_amd import block
    cases = []
    for p in X.PREFIX_LENS:
        prefix = X.prefix_bytes(p)
        for name, c, new in X.writer_blocks(prefix):
            cases += _caps(name, c, prefix, new)
    prefix = X.prefix_bytes(65536, 1)
    c, new = X.big_block(prefix)
    cases += [("1 MiB block behind 64 KiB", c, prefix, 65536 + len(new), None), ("1 MiB block behind 64 KiB, 1 short", c, prefix, 65536 + len(new) - 1, None)]
    plain = (O.fixture_plain("compression_66k_JSON") + O.fixture_plain("compression_65k")) * 3
    plain = plain[:len(plain) - 4321]
    for bs in (4, 5):
        rc, fr = O.frame_compress(plain, block_size=bs, block_mode=1)
        assert rc == 0
        blocks, bsize = X.frame_blocks(fr)
        so_far = b""
        for k, (compressed, data) in enumerate(blocks):
            if compressed:
                for tag, cap in (("", len(so_far) + bsize), (" exact", min(len(plain), len(so_far) + bsize))):
                    cases.append(("Linked frame block %d of %d KiB%s" % (k, bsize >> 10, tag), data, so_far, cap, None))
                so_far += O.decompress_prefix(data, so_far, len(so_far) + bsize)[1]
            else:
                so_far += data
        assert so_far == plain
    # throughput encoder, LZ4FLEX_BLOCK_HISTORY(h): 64 KiB blocks of one stream, block k > 0 with h bytes of the stream in front of it
    B = 65536
    stream = (plain * 3)[:8 * B]
    assert len(stream) == 8 * B
    for h in (32768, 65536):
        ks = list(range(8))
        in_off = np.array([k * B for k in ks], dtype=np.uint64)
        in_len = np.full(len(ks), B, dtype=np.uint32)
        flags = np.array([0] + [h << 8] * (len(ks) - 1), dtype=np.uint32)
        cap = O.max_out(B)
        outb = np.zeros(cap * len(ks), dtype=np.uint8)
        out_off = np.array([k * cap for k in ks], dtype=np.uint64)
        ol, st = block.compress_batch(np.frombuffer(stream, dtype=np.uint8), in_off, in_len, outb, out_off, np.full(len(ks), cap, dtype=np.uint32), flags=flags)
        assert (st == 0).all()
        reached = 0
        for k in ks:
            comp = outb[k * cap:k * cap + int(ol[k])].tobytes()
            pre = stream[max(0, k * B - h):k * B] if k else b""
            assert O.decompress_prefix(comp, pre, len(pre) + B) == ("ok", stream[k * B:(k + 1) * B]), (h, k)
            reached += k > 0 and O.decompress(comp, B)[0] != "ok"
            cases += [("throughput block %d, history %d" % (k, h), comp, pre, len(pre) + B, None),
                      ("throughput block %d, history %d, 40 short" % (k, h), comp, pre, len(pre) + B - 40, None)]
        assert reached, "no block of the history-mode stream reaches into its history"
    return Batch(cases)


def _run_and_check(env, batch, ctx, mem, what, chunk=None, second_pass=True):
    lib, L, torch = env
    if chunk is None:
        batch.check(batch.run(env, ctx, mem), mem != L.MEM_HOST, what, second_pass=second_pass)
        return
    for lo in range(0, batch.n, chunk):
        sub = Batch(batch.cases[lo:lo + chunk])
        sub.check(sub.run(env, ctx, mem), mem != L.MEM_HOST, what, second_pass=second_pass)


# ---------------------------------------------------------------- A: prefix mode, every decoder configuration
def test_prefix_mode_every_decoder(env, prefix_cases):
    lib, L, torch = env
    for v, par in _decoders(lib):
        for mem in (L.MEM_HOST, L.MEM_DEVICE):
            ctx = _ctx(lib, v, par)
            try:
                _run_and_check(env, prefix_cases, ctx, mem, "variant %d/%d mem %d" % (v, par, mem))
            finally:
                lib.lz4flex_ctx_destroy(ctx)


@pytest.mark.parametrize("variant", (7, 8))
@pytest.mark.parametrize("pair", (0, 2))
def test_prefix_mode_workgroup_decoder_paired(env, prefix_cases, variant, pair):
    """decompress_pcd_pair 2: every batch of <= 128 blocks gets a parser and a copier workgroup per block"""
    lib, L, torch = env
    ctx = _ctx(lib, variant, decompress_pcd_pair=pair)
    try:
        _run_and_check(env, prefix_cases, ctx, L.MEM_DEVICE, "variant %d pair %d" % (variant, pair), chunk=128)
    finally:
        lib.lz4flex_ctx_destroy(ctx)


@pytest.mark.parametrize("variant", (7, 13))
def test_prefix_mode_the_kernel_decodes_every_valid_block_itself(env, prefix_cases, variant):
    """second pass off: every valid prefix block comes out of the workgroup / sequence decoder itself, invalid ones stay marked"""
    lib, L, torch = env
    ctx = _ctx(lib, variant, decompress_second_pass=0)
    try:
        res = prefix_cases.run(env, ctx, L.MEM_DEVICE)
        prefix_cases.check(res, True, "variant %d, second pass off" % variant, second_pass=False)
        for i, w in enumerate(prefix_cases.want):
            assert int(res[2][i]) == (0 if w[0] == "ok" else REDO), (prefix_cases.cases[i][0], int(res[2][i]), w[0])
    finally:
        lib.lz4flex_ctx_destroy(ctx)


# ---------------------------------------------------------------- the fix: out_pos > out_cap
def _beyond_cases():
    """blocks whose sink position lies behind the sink's end; the regions leave room for the whole block behind out_pos, so that even
    a kernel without the check would only write canary bytes of this test's own buffer"""
    out = []
    for p in (1, 17, 1000, 70000):
        prefix = X.prefix_bytes(p, 5)
        for name, c, new in X.writer_blocks(prefix)[:6]:
            for cap in (0, p - 1, p // 2):
                out.append(("%s, cap %d < out_pos" % (name, cap), c, prefix, cap, None))
            out.append(("%s, cap == out_pos" % name, c, prefix, p, None))
    return out


def test_sink_position_behind_the_sink_end(env):
    """out_pos > out_cap: status INVALID_ARG, out_len 0, detail 0, nothing written -- every decoder, device memory first, then host"""
    lib, L, torch = env
    cases = _beyond_cases()
    # (an unchecked kernel would decode the whole block from out_pos on: the block's output plus the wide stores' 16 bytes fit in the slack)
    longest = max(len(O.decompress_prefix(c[1], c[2], len(c[2]) + (1 << 20))[1]) for c in cases)
    batch = Batch(cases, slack=longest + 4096)
    assert sum(w[0] == "InvalidArg" for w in batch.want) >= 40
    for mem in (L.MEM_DEVICE, L.MEM_HOST):
        for v, par in _decoders(lib) + [(0, 0)]:
            ctx = _ctx(lib, v, par)
            try:
                batch.check(batch.run(env, ctx, mem), mem != L.MEM_HOST, "variant %d/%d mem %d" % (v, par, mem))
            finally:
                lib.lz4flex_ctx_destroy(ctx)


# ---------------------------------------------------------------- B: prefix mode, default dispatch by batch size
def _thresholds(lib):
    out = []
    for i in range(64):
        v = lib.lz4flex_get_tuning(None, b"dispatch_threshold_%d" % i)
        if v < 0:
            break
        out.append(v)
    assert 640 in out and 14336 in out, out
    return out


def test_prefix_mode_default_dispatch_by_size(env):
    """every dispatch threshold T - 1, T, T + 1: small blocks behind prefixes of up to 8 KiB, device memory, the default decoder; the same
    with LZ4FLEX_MEM_BIG_BLOCKS (results do not depend on the hint)"""
    lib, L, torch = env
    rnd = random.Random(31)
    src = O.fixture_plain("compression_66k_JSON") + O.fixture_plain("compression_65k")
    pool = []
    for k in range(240):
        a = rnd.randrange(len(src) - 17000)
        p = rnd.choice((0, 1, 15, 16, 17, 1279, 1281, 3584, rnd.randint(0, 8192)))
        n = rnd.randint(2048, 8192)
        prefix, data = src[a:a + p], src[a + p:a + p + n]
        if k % 3 == 2:
            w = Writer(k, prefix)
            while len(w.out) - w.base < n - 300:
                lit = rnd.randint(0, 12)
                w.seq(lit, rnd.randint(1, min(len(w.out) + lit, 65535)), rnd.randint(4, 80))
            c, data = w.end(5)
        else:
            c = O.compress_with_dict(data, prefix) if p > 3 else O.compress(data)
        cap = len(prefix) + len(data) + (777 if k % 5 == 0 else 0)
        pool.append((c, prefix, cap, data))
    sizes = sorted({n for t in _thresholds(lib) for n in (t - 1, t, t + 1) if n >= 1})
    nmax = max(sizes)
    cases = []
    for i in range(nmax):
        c, prefix, cap, data = pool[i % len(pool)]
        cases.append(("pool %d (block %d)" % (i % len(pool), i), c, prefix, cap, None, ("ok", data)))
    for c, prefix, cap, data in pool:
        assert O.decompress_prefix(c, prefix, cap) == ("ok", data)
    batch = Batch(cases, misalign=0)
    ctx = _ctx(lib)
    try:
        for n in sizes:
            for flags in (0, L.MEM_BIG_BLOCKS):
                batch.check(batch.run(env, ctx, L.MEM_DEVICE, flags=flags, n=n), True, "%d blocks, flags %#x" % (n, flags), n=n)
    finally:
        lib.lz4flex_ctx_destroy(ctx)


# ---------------------------------------------------------------- C: one chain
LENS = (0, 1, 17, 65539, 300, 0, 5000, 70000, 17, 1, 40000, 65536, 3, 20000)


def _chain(pre, lens, seed):
    """a chain: `pre` bytes before it, then blocks of the given new lengths whose matches reach up to 65 535 bytes back, across
    as many earlier blocks as that is"""
    rnd = random.Random(seed)
    stream = X.prefix_bytes(pre, seed)
    blocks = []
    for j, n in enumerate(lens):
        w = Writer(seed * 1000 + j, stream)
        if n >= 40:
            while len(w.out) - w.base < n - 30:
                room = n - 30 - (len(w.out) - w.base)
                lit = rnd.randint(0, min(8, room))
                reach = min(len(w.out) + lit, 65535)
                off = rnd.choice((reach, rnd.randint(1, reach), rnd.randint(1, min(reach, 64))))
                ml = min(max(4, room - lit), rnd.choice((4, 12, 100, 1000, 4000)))
                if ml < 4 or lit + ml > room + 4:
                    break
                w.seq(lit, off, ml)
        c, new = w.end(n - (len(w.out) - w.base))
        assert len(new) == n
        blocks.append((c, new))
        stream = stream + new
    return X.prefix_bytes(pre, seed), blocks


def _chain_batch(pre, blocks, bad_at=None):
    """the blocks of one chain as a batch; block `bad_at` replaced by one whose match reaches one byte behind its prefix
    (OffsetOutOfBounds), or by a literal run that runs out of input.  Returns the batch and how many of its blocks are specified"""
    cases, prefix = [], pre
    for j, (c, new) in enumerate(blocks):
        if j == bad_at:
            c = Writer(7, prefix).seq(3, 3, 4).bad_seq(0, len(prefix) + 8, 4).end(3)[0] if len(prefix) + 8 <= 65535 else b"\x1f"
        cases.append(("chain block %d (%d new bytes)" % (j, len(new)), c, prefix, len(prefix) + len(new), None))
        prefix = prefix + new
    b = Batch(cases, chain=pre)
    if bad_at is None:
        return b, len(blocks)
    b.dont_care_from = int(b.out_off[0]) + int(b.pos[bad_at])          # its own sink and everything behind it
    return b, bad_at + 1


@pytest.mark.parametrize("variant", (0, 8))
def test_one_chain(env, variant):
    """MEM_CHAINED: ragged blocks (0, 1, 17, 65 539 ... new bytes), bytes before the chain or none, a block that gives up at the first,
    a middle and the last block (the ordered second pass), an invalid block in the middle (the blocks before it and its own verdict)"""
    lib, L, torch = env
    for pre in (0, 1000):
        raw_pre, blocks = _chain(pre, LENS, 3 + pre)
        full, _ = _chain_batch(raw_pre, blocks)
        assert full.want == [("ok", new) for _, new in blocks]
        for mem in (L.MEM_HOST, L.MEM_DEVICE):
            for giveup in (0, 1, len(blocks) // 2, len(blocks)):
                ctx = _ctx(lib, variant, debug_chain_giveup=giveup)
                try:
                    full.check(full.run(env, ctx, mem, flags=L.MEM_CHAINED), mem != L.MEM_HOST, "chain, pre %d, mem %d, giveup %d" % (pre, mem, giveup))
                finally:
                    lib.lz4flex_ctx_destroy(ctx)
            for bad_at in (2, 7):
                b, n_spec = _chain_batch(raw_pre, blocks, bad_at)
                assert b.want[bad_at][0] not in ("ok", "InvalidArg")
                ctx = _ctx(lib, variant)
                try:
                    b.check(b.run(env, ctx, mem, flags=L.MEM_CHAINED), mem != L.MEM_HOST, "chain, invalid block %d, mem %d" % (bad_at, mem), n=n_spec)
                finally:
                    lib.lz4flex_ctx_destroy(ctx)


def test_one_chain_with_a_sink_position_behind_its_end(env):
    """a chained block with out_pos > out_cap ends its chain like a decode error: INVALID_ARG, nothing written; the blocks before it are
    decoded"""
    lib, L, torch = env
    raw_pre, blocks = _chain(100, LENS[:8], 11)
    bad_at = 4
    b, _ = _chain_batch(raw_pre, blocks)
    b.cap[bad_at] = b.pos[bad_at] - 1
    b.want[bad_at] = ("InvalidArg",)
    for mem in (L.MEM_DEVICE, L.MEM_HOST):
        # behind it nothing is specified.  Its own place, [out_pos, next block's out_pos), stays untouched on the device; a HOST chain
        # comes back in one transfer up to the end of its last good block, so there the place holds whatever the staging area held
        b.dont_care_from = int(b.out_off[0]) + int(b.pos[bad_at + 1 if mem == L.MEM_DEVICE else bad_at])
        ctx = _ctx(lib)
        try:
            b.check(b.run(env, ctx, mem, flags=L.MEM_CHAINED), mem != L.MEM_HOST, "chain with out_pos > cap, mem %d" % mem, n=bad_at + 1)
        finally:
            lib.lz4flex_ctx_destroy(ctx)


# ---------------------------------------------------------------- D: several chains (chain_prev), device only
def _multi_chain_batch(n_chains, seed=5):
    """n_chains chains of 1 ... 4 blocks (unequal depth), every chain with one block of 0 new bytes, blocks in level order"""
    templates = []
    for t in range(48):
        depth = 1 + t % 4
        lens = [random.Random(seed * 100 + t * 7 + j).randint(1, 6000) for j in range(depth)]
        lens[t % depth] = 0
        templates.append(_chain(t * 37 % 300, lens, seed * 1000 + t))
    chains = [templates[c % len(templates)] for c in range(n_chains)]
    order = [(c, j) for j in range(4) for c in range(n_chains) if j < len(chains[c][1])]
    cases, prev, idx, region = [], [], {}, {}
    off = 0
    init_parts = []
    for c, (pre, blocks) in enumerate(chains):
        total = len(pre) + sum(len(new) for _, new in blocks)
        region[c] = off
        init_parts.append((off, pre))
        off += total + CANARY
    for k, (c, j) in enumerate(order):
        pre, blocks = chains[c]
        prefix = pre + b"".join(new for _, new in blocks[:j])
        cases.append(("chain %d block %d" % (c, j), blocks[j][0], prefix, len(prefix) + len(blocks[j][1]), None, ("ok", blocks[j][1])))
        prev.append(idx[(c, j - 1)] if j else 0xFFFFFFFF)
        idx[(c, j)] = k
    b = Batch(cases, chain=b"")
    b.out_off = np.array([region[c] for c, _ in order], dtype=np.uint64)
    b.init = np.full(off + 64, FILL, dtype=np.uint8)
    for o, pre in init_parts:
        b.init[o:o + len(pre)] = np.frombuffer(pre, dtype=np.uint8)
    return b, np.array(prev, dtype=np.uint32)


@pytest.mark.parametrize("n_chains", (1, 256, 257, 512, 513, 1024))
def test_several_chains(env, n_chains):
    lib, L, torch = env
    b, prev = _multi_chain_batch(n_chains)
    ctx = _ctx(lib)
    try:
        for hint in (n_chains, 0):
            res = b.run(env, ctx, L.MEM_DEVICE, flags=L.MEM_CHAINED, chain_prev=prev, n_chains=hint)
            b.check(res, True, "%d chains, hint %d" % (n_chains, hint))
    finally:
        lib.lz4flex_ctx_destroy(ctx)


# ---------------------------------------------------------------- E: dictionary mode
def _dict_cases():
    out = []
    for dl in (0, 1, 5, 1000, 65535, 65536, 70000):
        d = X.prefix_bytes(dl, 9)
        for name, c, new in X.writer_blocks(d, seed=2)[:12]:
            # the writer's prefix is the dictionary here: the sink starts empty, offsets beyond the output reach the dictionary
            if new is not None:
                out.append(("dict %d: %s" % (dl, name), c, b"", len(new), d))
                out.append(("dict %d: %s, 1 short" % (dl, name), c, b"", max(len(new) - 1, 0), d))
            else:
                out.append(("dict %d: %s" % (dl, name), c, b"", 100, d))
        # a dictionary AND a prefix (the reference-order kernel takes both): offsets beyond the prefix reach the dictionary
        for p in (0, 3, 1500):
            prefix = X.prefix_bytes(p, 10)
            w = Writer(dl + p, d + prefix)
            w.seq(2, min(dl + p + 2, 65535) if dl + p else 2, 40)
            for k in range(20):
                lit = k % 5
                w.seq(lit, 1 + (k * 7919) % min(len(w.out) + lit, 65535), 4 + k)
            c, new = w.end(5)
            out.append(("dict %d + prefix %d" % (dl, p), c, prefix, p + len(new), d))
            if dl + p + 1 <= 65535:
                c2, _ = Writer(3, d + prefix).bad_seq(0, dl + p + 1, 4).end(3)
                out.append(("dict %d + prefix %d, one byte too far" % (dl, p), c2, prefix, p + 50, d))
    return out


def test_dictionary_mode(env):
    lib, L, torch = env
    cases = _dict_cases()
    batch = Batch(cases)
    assert sum(w[0] == "ok" for w in batch.want) >= 90 and sum(w[0] == "OffsetOutOfBounds" for w in batch.want) >= 10
    for variant in (0, 1, 7, 13):
        for mem in (L.MEM_HOST, L.MEM_DEVICE):
            ctx = _ctx(lib, variant)
            try:
                batch.check(batch.run(env, ctx, mem), mem != L.MEM_HOST, "dictionary, variant %d, mem %d" % (variant, mem))
            finally:
                lib.lz4flex_ctx_destroy(ctx)


# ---------------------------------------------------------------- F: API misuse, refused before any launch
def test_misuse_is_refused(env):
    lib, L, torch = env
    dev = torch.device("cuda", 0)
    host = dict(z64=np.zeros(70000, dtype=np.uint64), z32=np.zeros(70000, dtype=np.uint32), o32=np.ones(70000, dtype=np.uint32),
                inb=np.zeros(64, dtype=np.uint8), out=np.zeros(64, dtype=np.uint8))
    for mem in (L.MEM_HOST, L.MEM_DEVICE):
        if mem == L.MEM_HOST:
            ptr = {k: C.c_void_p(v.ctypes.data) for k, v in host.items()}
            stream = None
        else:
            keep = {k: torch.from_numpy(v.view(np.uint8).reshape(-1)).to(dev) for k, v in host.items()}
            ptr = {k: C.c_void_p(v.data_ptr()) for k, v in keep.items()}
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()

        def call(n, ext):
            return lib.lz4flex_decompress_batch_ex(ctx, ptr["inb"], ptr["z64"], ptr["o32"], n, ptr["out"], ptr["z64"], ptr["o32"],
                                                   ptr["z32"], ptr["z32"], ptr["z64"], ext, mem | L.MEM_CHAINED, stream)
        ctx = _ctx(lib)
        try:
            ext = L.DecompressExt()
            assert call(2, C.byref(ext)) == -INVALID_ARG             # chained without out_pos
            assert call(2, None) == -INVALID_ARG                     # chained without ext
            ext.out_pos = ptr["z32"]
            ext.dict_base, ext.dict_off, ext.dict_len = ptr["inb"], ptr["z64"], ptr["z32"]
            assert call(2, C.byref(ext)) == -INVALID_ARG             # chained with a dictionary
            ext.dict_base = ext.dict_off = ext.dict_len = None
            assert call(65537, C.byref(ext)) == -INVALID_ARG         # chained, more than 65 536 blocks
        finally:
            lib.lz4flex_ctx_destroy(ctx)
    # chain_prev belongs to MEM_DEVICE | MEM_CHAINED batches only.  In any other batch the member is not read -- it lies behind the four
    # members that callers built against an older header hand over (lz4flex_decompress_batch_ex) -- and the batch decodes as without it
    plain = Batch([("a", b"\x30abc", b"xy", 5, None), ("b", b"\x30def", b"", 3, None)])
    raw_pre, blocks = _chain(5, (3, 40, 0, 7), 21)
    chained, _ = _chain_batch(raw_pre, blocks)
    for mem, flags, b in ((L.MEM_HOST, L.MEM_CHAINED, chained), (L.MEM_HOST, 0, plain), (L.MEM_DEVICE, 0, plain)):
        ctx = _ctx(lib)
        try:
            res = b.run(env, ctx, mem, flags=flags, chain_prev=np.full(b.n, 0xFFFFFFFF, dtype=np.uint32), n_chains=5)
            b.check(res, mem != L.MEM_HOST, "chain_prev outside device chains, mem %d flags %#x" % (mem, flags))
        finally:
            lib.lz4flex_ctx_destroy(ctx)
