"""GPU (-m gpu): lz4flex_decompress_batch_shared_dict -- n blocks decoded against ONE dictionary by the sequence decoder's dictionary
form (lz4_decompress_seq.hip: the dictionary is a virtual prefix in front of every block's output, read from its own buffer).

Checker: the oracle's decompress_into_with_dict (oracle_api.decompress): status, out_len, the bytes, the OutputTooSmall {expected,
actual} detail; and lz4flex_decompress_batch_ex with per-block arrays that name the same dictionary for every block, whose results the
entry promises to give.  Every sink lies between canaries, so does the dictionary, which is compared with its copy after every call."""
import ctypes as C

import numpy as np
import pytest

import dict_cases as D
import oracle_api as O
from lz4_writer import Writer

pytestmark = pytest.mark.gpu
REDO = 0x7F000001
CANARY = 64
FILL = 0xA5
ERR_CODES = {v: k for k, v in O.ERR_NAMES.items()}
KEEP = 1280                      # the sequence decoder's window history (lz4_decompress_seq.hip LZ4S_KEEP)


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


def parse(comp):
    """(position, offset, match length) of every match of a well-formed block"""
    out, ip, op, n = [], 0, 0, len(comp)
    while ip < n:
        t = comp[ip]
        ip += 1
        lit = t >> 4
        if lit == 15:
            while True:
                b = comp[ip]
                ip += 1
                lit += b
                if b != 255:
                    break
        ip += lit
        op += lit
        if ip >= n:
            break
        off = comp[ip] | (comp[ip + 1] << 8)
        ip += 2
        ml = 4 + (t & 15)
        if ml == 19:
            while True:
                b = comp[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        out.append((op, off, ml))
        op += ml
    return out


def reaches_dict(comps):
    return any(off > pos for c in comps for pos, off, _ in parse(c))


class Batch:
    """cases: (name, block, cap[, alloc]) against the one dictionary `dic`.  Sink i: CANARY bytes of FILL, min(cap, alloc) bytes, CANARY bytes
    of FILL, at an out_off that is no multiple of 16.  `want` is the oracle's verdict (a sink larger than its allocation -- alloc -- is
    judged at the allocation's size, which the block must fit)."""

    def __init__(self, cases, dic, want=None):
        self.cases, self.dic, self.n = cases, bytes(dic), len(cases)
        n = self.n
        comps = [c[1] for c in cases]
        self.in_len = np.array([len(c) for c in comps], dtype=np.uint32)
        self.in_off = (np.concatenate([[0], np.cumsum(self.in_len[:-1], dtype=np.uint64)]) + 3).astype(np.uint64)
        self.inb = np.frombuffer(bytes(3) + b"".join(comps) + bytes(64), dtype=np.uint8).copy()
        self.cap = np.array([c[2] for c in cases], dtype=np.uint32)
        self.alloc = [min(c[2], c[3]) if len(c) > 3 else c[2] for c in cases]
        self.want = want if want is not None else [O.decompress(c[1], a, dict_data=self.dic) for c, a in zip(cases, self.alloc)]
        off, o = [], 0
        for a in self.alloc:
            o += CANARY
            if o % 16 == 0:
                o += 5
            off.append(o)
            o += a + CANARY
        self.out_off = np.array(off, dtype=np.uint64)
        self.init = np.full(o + 64, FILL, dtype=np.uint8)
        self.dictb = np.frombuffer(bytes([0x5A]) * (CANARY + 1) + self.dic + bytes([0x5A]) * CANARY, dtype=np.uint8).copy()
        self.dict_at = CANARY + 1

    def expected(self, loose):
        """the image the output buffer must have, and where it must have it.  loose (device batches decoded in the reference's order, as
        lz4flex_decompress_batch_ex decodes them): dword stores may rewrite bytes behind a block's end, inside its sink"""
        exp = self.init.copy()
        care = np.ones(len(exp), dtype=bool)
        for i, w in enumerate(self.want):
            o, a = int(self.out_off[i]), self.alloc[i]
            if w[0] == "ok":
                exp[o:o + len(w[1])] = np.frombuffer(w[1], dtype=np.uint8)
                if loose:
                    care[o + len(w[1]):o + a] = False
            elif loose is not None:
                care[o:o + a] = False                          # a failed block may have written part of its sink (device memory)
        return exp, care

    def run(self, env, ctx, mem, entry="shared", stream=None, sync=True):
        lib, L, torch = env
        n = self.n
        out = self.init.copy()
        out_len = np.full(n, 0xDEADBEEF, dtype=np.uint32)
        status = np.full(n, -1, dtype=np.int32)
        detail = np.full((n, 2), 0xEE, dtype=np.uint64)
        arrays = dict(inb=self.inb, in_off=self.in_off, in_len=self.in_len, out=out, out_off=self.out_off, cap=self.cap,
                      out_len=out_len, status=status, detail=detail, dictb=self.dictb.copy())
        if entry == "ex":
            arrays.update(dict_off=np.zeros(n, dtype=np.uint64), dict_len=np.full(n, len(self.dic), dtype=np.uint32))
        if mem == L.MEM_HOST:
            keep = arrays
            addr = {k: v.ctypes.data for k, v in arrays.items()}
            sp = None
        else:
            dev = torch.device("cuda", 0)
            keep = {k: torch.from_numpy(v.view(np.uint8).reshape(-1)).to(dev) for k, v in arrays.items()}
            addr = {k: v.data_ptr() for k, v in keep.items()}
            sp = C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        ptr = {k: C.c_void_p(v) for k, v in addr.items()}
        dptr = C.c_void_p(addr["dictb"] + self.dict_at)
        if entry == "ex":
            ext = L.DecompressExt(dptr, ptr["dict_off"], ptr["dict_len"], None, None, 0)
            rc = lib.lz4flex_decompress_batch_ex(ctx, ptr["inb"], ptr["in_off"], ptr["in_len"], n, ptr["out"], ptr["out_off"], ptr["cap"],
                                                 ptr["out_len"], ptr["status"], ptr["detail"], C.byref(ext), mem, sp)
        else:
            rc = lib.lz4flex_decompress_batch_shared_dict(ctx, ptr["inb"], ptr["in_off"], ptr["in_len"], n, ptr["out"], ptr["out_off"], ptr["cap"],
                                                          ptr["out_len"], ptr["status"], ptr["detail"], dptr, len(self.dic), mem, sp)
        assert rc == 0, (rc, L.last_error())

        def fetch():
            if mem != L.MEM_HOST:
                torch.cuda.synchronize()
                for k in ("out", "out_len", "status", "detail", "dictb"):
                    arrays[k].view(np.uint8).reshape(-1)[:] = keep[k].cpu().numpy()
            assert np.array_equal(arrays["dictb"], self.dictb), "the dictionary or the bytes around it were written"
            return out, out_len, status, detail
        return fetch() if sync else fetch

    def check(self, res, loose, what, second_pass=True):
        out, out_len, status, detail = res
        for i in range(self.n):
            name, w = self.cases[i][0], self.want[i]
            st, ol = int(status[i]), int(out_len[i])
            if w[0] == "ok":
                assert st == 0 and ol == len(w[1]), (what, name, st, ol, len(w[1]))
                assert tuple(int(v) for v in detail[i]) == (0, 0), (what, name)
            elif not second_pass:
                assert st == REDO and ol == 0, (what, name, hex(st), w)
            else:
                assert st == ERR_CODES[w[0]] and ol == 0, (what, name, st, w)
                want_det = (w[1][0], int(self.cap[i])) if w[0] == "OutputTooSmall" else (0, 0)
                assert tuple(int(v) for v in detail[i]) == want_det, (what, name, detail[i], w)
        exp, care = self.expected(loose)
        bad = np.nonzero((out != exp) & care)[0]
        if len(bad):
            b = int(bad[0])
            i = int(np.searchsorted(self.out_off, b, side="right")) - 1
            raise AssertionError("%s: %d wrong bytes, first at %d = sink %d (%s) + %d" %
                                 (what, len(bad), b, i, self.cases[max(i, 0)][0], b - int(self.out_off[max(i, 0)])))


def same_results(a, b, batch, what):
    """two runs gave the same out_len / status / detail and the same bytes for every decoded block"""
    for k in (1, 2, 3):
        assert np.array_equal(a[k], b[k]), (what, ("out_len", "status", "detail")[k - 1])
    for i in range(batch.n):
        if int(a[2][i]) == 0:
            o, n = int(batch.out_off[i]), int(a[1][i])
            assert np.array_equal(a[0][o:o + n], b[0][o:o + n]), (what, batch.cases[i][0])


# ---------------------------------------------------------------- 1. real data, both encoders, equality with lz4flex_decompress_batch_ex
_pool = {}


def pool(kind):
    """8 blocks of one kind -- 4 KiB and 64 KiB, two of each from this library's shared-dictionary encoder and two from the oracle's
    compress_with_dict -- and their dictionary (70 000 bytes: more than an offset reaches)"""
    if kind not in _pool:
        from lz4_flex_amd import block
        dic = D.dictionary(kind)[:70000]
        plains = [D.block(kind, n, salt) for salt, n in enumerate((4096, 65536, 4096, 65536, 4096, 65536, 4096, 65536))]
        items = [("%s-oracle-%d" % (kind, i), O.compress_with_dict(p, dic), p) for i, p in enumerate(plains[:4])]
        rest = plains[4:]
        src = np.frombuffer(b"".join(rest), dtype=np.uint8)
        lens = [len(p) for p in rest]
        offs = np.concatenate([[0], np.cumsum(lens[:-1])])
        caps = [O.max_out(n) for n in lens]
        ooff = np.concatenate([[0], np.cumsum(caps[:-1])])
        outb = np.zeros(sum(caps), dtype=np.uint8)
        olen, st = block.compress_batch_with_shared_dict(src, offs, lens, np.frombuffer(dic, dtype=np.uint8), outb, ooff, caps)
        assert not st.any()
        for i, p in enumerate(rest):
            comp = outb[int(ooff[i]):int(ooff[i]) + int(olen[i])].tobytes()
            assert D.oracle_decodes(comp, p, dic)
            items.append(("%s-lib-%d" % (kind, i), comp, p))
        _pool[kind] = (dic, items)
    return _pool[kind]


_batches = {}


def real_batch(kind, n):
    if (kind, n) not in _batches:
        dic, items = pool(kind)
        cases, want = [], []
        for i in range(n):
            k = (i * 3 + i // 8) % 8
            if n > 100 and i % 16 != 5:
                k &= ~1                                    # (a large batch: mostly the 4 KiB blocks, the even items)
            name, comp, plain = items[k]
            cases.append((name, comp, len(plain) + (0 if i % 2 == 0 else 1 + i % 37)))     # out_cap exact and larger
            want.append(("ok", plain))
        _batches[(kind, n)] = Batch(cases, dic, want=want)
    return _batches[(kind, n)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 3000])
@pytest.mark.parametrize("kind", D.KINDS)
def test_equals_batch_ex(env, kind, n):
    lib, L, torch = env
    b = real_batch(kind, n)
    if kind not in ("random",):
        assert reaches_dict([c[1] for c in b.cases[:8]]), "no block of the batch references the dictionary"
    ctx, raw = _ctx(lib), _ctx(lib, decompress_second_pass=0)
    try:
        for mem in (L.MEM_DEVICE, L.MEM_HOST):
            what = "%s n=%d mem=%d" % (kind, n, mem)
            got = b.run(env, ctx, mem)
            b.check(got, False if mem == L.MEM_DEVICE else None, what)
            ex = b.run(env, ctx, mem, entry="ex")
            b.check(ex, True if mem == L.MEM_DEVICE else None, what + " (batch_ex)")
            same_results(got, ex, b, what)
        # 4. second pass off: the dictionary form decodes every valid block itself
        b.check(b.run(env, raw, L.MEM_DEVICE), False, "%s n=%d second pass off" % (kind, n), second_pass=False)
    finally:
        lib.lz4flex_ctx_destroy(ctx)
        lib.lz4flex_ctx_destroy(raw)


# ---------------------------------------------------------------- 2. dictionary lengths
DICT_LENS = [1, 3, 4, 15, 16, 17, KEEP - 1, KEEP, KEEP + 1, 4096, 32768, 65535, 65536, 65537, 200000]


@pytest.mark.parametrize("dlen", DICT_LENS)
def test_dictionary_lengths(env, dlen):
    lib, L, torch = env
    text = D.dictionary("text")
    dic = text[300000 - dlen:300000]
    reach = min(dlen, 65535)
    # text that repeats the dictionary's end and goes on: the oracle's encoder finds its matches in the dictionary
    plains = [dic[-min(dlen, 3000):] + D.block("text", 4096, 1), dic[-min(dlen, 40000):] + D.block("text", 65536, 2), D.block("text", 4096, 3)]
    cases = [("oracle-%d" % i, O.compress_with_dict(p, dic), len(p) + (i % 2) * 9) for i, p in enumerate(plains)]
    # and two written by hand: the oldest byte an offset reaches, at position 0 and behind literals
    w = Writer(seed=dlen, prefix=dic).seq(0, reach, 4 if reach >= 4 else 40).seq(7, min(reach + 11, 65535), 30)
    comp, plain = w.end(3)
    cases.append(("oldest", comp, len(plain)))
    w = Writer(seed=dlen + 1, prefix=dic).seq(0, min(reach, 17), 5000).seq(2, min(reach + 5002, 65535), 70)
    comp, plain = w.end(0)
    cases.append(("straddle", comp, len(plain) + 3))
    assert reaches_dict([c[1] for c in cases])
    if dlen >= KEEP - 1:
        assert reaches_dict([c[1] for c in cases[:3]]), "the oracle's encoder did not use the dictionary"
    b = Batch(cases, dic)
    assert all(w[0] == "ok" for w in b.want)
    ctx, raw = _ctx(lib), _ctx(lib, decompress_second_pass=0)
    try:
        got = b.run(env, ctx, L.MEM_DEVICE)
        b.check(got, False, "dict_len %d" % dlen)
        same_results(got, b.run(env, ctx, L.MEM_DEVICE, entry="ex"), b, "dict_len %d against batch_ex" % dlen)
        b.check(b.run(env, ctx, L.MEM_HOST), None, "dict_len %d host" % dlen)
        b.check(b.run(env, raw, L.MEM_DEVICE), False, "dict_len %d second pass off" % dlen, second_pass=False)
    finally:
        lib.lz4flex_ctx_destroy(ctx)
        lib.lz4flex_ctx_destroy(raw)


# ---------------------------------------------------------------- 3. blocks written by hand: one wavefront's corner cases
HAND_DICT = Writer(seed=4242).end(6000)[1]           # 6 000 bytes of noise: longer than the window (3 584), shorter than an offset's reach
TOTALS = [4, 16, 17, 64, 65, 273, 274, 1023, 1024, 70000]
SIDES = [1, 15, 16, 17]


def hand_cases():
    dic, dl = HAND_DICT, len(HAND_DICT)
    cases = []

    def add(name, w, tail=5, cap_extra=0, alloc=None):
        comp, plain = w.end(tail)
        cases.append((name, comp, len(plain) + cap_extra) if alloc is None else (name, comp, len(plain) + cap_extra, alloc))
        return comp, plain

    W = lambda seed: Writer(seed=seed, prefix=dic)     # noqa: E731
    add("inside-dict-first", W(1).seq(0, 100, 20))
    add("inside-dict-first-off-eq-len", W(2).seq(0, 100, 100))
    add("inside-dict-far", W(3).seq(0, 5000, 64).seq(3, 5500, 65).seq(1, 4000, 16))
    add("oldest-at-0", W(4).seq(0, dl, 40))
    add("oldest-behind-10", W(5).seq(10, dl + 10, 40))
    add("oldest-behind-4000", W(6).seq(0, 300, 3990).seq(10, dl + 4000, 33))
    add("beyond-oldest-at-0", W(7).bad_seq(0, dl + 1, 40))
    add("beyond-oldest-behind-10", W(8).bad_seq(10, dl + 11, 40))
    add("beyond-oldest-later", W(9).seq(4, 50, 30).seq(6, 40, 8).bad_seq(3, dl + 4 + 30 + 6 + 8 + 3 + 1, 12))
    for T in TOTALS:
        for d in SIDES:
            if d >= T:
                continue
            p = T - d + 3                                  # literals in front: the source ends in front of the match (offset >= length)
            if p + d <= 65535:
                add("straddle-%d-dict-%d" % (T, d), W(100 + T + d).seq(p, p + d, T))
            add("straddle-%d-dict-%d-overlap" % (T, d), W(200 + T + d).seq(0, d, T))      # offset < length: runs into its own output
            add("straddle-%d-dict-%d-overlap-lit" % (T, d), W(300 + T + d).seq(2, d + 2, T), tail=0)
    for p in (64, 65, 1024):
        add("lit-%d-straddle" % p, W(400 + p).seq(p, p + 5, 40))
        add("lit-%d-straddle-overlap" % p, W(500 + p).seq(p, p + 5, p + 15))
        add("lit-%d-straddle-long" % p, W(600 + p).seq(p, p + 700, 1500))
    # far matches (their source has left the window: > 3.5 KiB of output behind the dictionary) whose 16-byte loads cross the boundary
    for d in (1, 5, 15, 16, 17, 40, 63, 64):
        for ml in (4, 16, 20, 64):
            add("far-%d-dict-%d" % (ml, d), W(700 + d + ml).seq(9, 200, 30).seq(0, 1, 5000).seq(3, 5042 + d, ml).seq(1, 5043 + ml + d + 20, 24))
    add("far-just-behind", W(800).seq(0, 1, 6000).seq(3, 6003, 32).seq(2, 6030, 64))
    add("long-from-dict", W(801).seq(0, 2000, 1900).seq(5, 3000, 1024).seq(0, 1100, 3000))
    add("long-straddle-far", W(802).seq(0, 7, 4500).seq(1, 4501 + 600, 2000))
    cases.append(("empty", b"", 16))
    comp, plain = W(900).seq(3, 50, 30).seq(200, 100, 400).end(5)
    cases.append(("one-byte-short", comp, len(plain) - 1))
    cases.append(("one-byte-short-in-match", comp, 3 + 30 + 200 + 399))
    comp, plain = W(901).seq(1, 7, 9).end(2)
    cases.append(("cap-max", comp, 0xFFFFFFFF, len(plain) + 20))
    return cases


_hand = []


def hand_batch():
    if not _hand:
        _hand.append(Batch(hand_cases(), HAND_DICT))
    return _hand[0]


def test_hand_cases_say_what_they_mean():
    b = hand_batch()
    verdict = {c[0]: w[0] for c, w in zip(b.cases, b.want)}
    assert verdict["beyond-oldest-at-0"] == verdict["beyond-oldest-behind-10"] == verdict["beyond-oldest-later"] == "OffsetOutOfBounds"
    assert verdict["empty"] == "ExpectedAnotherByte"
    assert verdict["one-byte-short"] == verdict["one-byte-short-in-match"] == "OutputTooSmall"
    bad = {"beyond-oldest-at-0", "beyond-oldest-behind-10", "beyond-oldest-later", "empty", "one-byte-short", "one-byte-short-in-match"}
    assert all(v == "ok" for k, v in verdict.items() if k not in bad)
    for c, w in zip(b.cases, b.want):               # the writer's plain text is the oracle's
        if c[0].startswith("straddle-70000"):
            assert len(w[1]) >= 70000


@pytest.mark.parametrize("mem", ["device", "host"])
def test_hand_written_blocks(env, mem):
    lib, L, torch = env
    b = hand_batch()
    m = L.MEM_DEVICE if mem == "device" else L.MEM_HOST
    ctx = _ctx(lib)
    try:
        got = b.run(env, ctx, m)
        b.check(got, False if mem == "device" else None, "hand " + mem)
        same_results(got, b.run(env, ctx, m, entry="ex"), b, "hand %s against batch_ex" % mem)
    finally:
        lib.lz4flex_ctx_destroy(ctx)


def test_hand_written_blocks_second_pass_off(env):
    """4.: the dictionary form marks what the reference rejects or what does not fit, and nothing else"""
    lib, L, torch = env
    b = hand_batch()
    raw = _ctx(lib, decompress_second_pass=0)
    try:
        b.check(b.run(env, raw, L.MEM_DEVICE), False, "hand second pass off", second_pass=False)
    finally:
        lib.lz4flex_ctx_destroy(raw)


# ---------------------------------------------------------------- 5. A/B
def mixed_batch():
    dic, items = pool("text")
    cases = []
    for i in range(96):
        name, comp, plain = items[i % 8]
        k = i % 6
        if k == 1:
            cases.append((name + "-truncated", comp[:len(comp) * 2 // 3], len(plain)))
        elif k == 3:
            cases.append((name + "-short-sink", comp, len(plain) - 1 - i))
        elif k == 4:
            matches = parse(comp)                          # (a 4 KiB block that repeats the dictionary is a handful of sequences)
            pos = matches[min(5, len(matches) - 1)]
            cut = bytearray(comp)
            at = comp.rindex(bytes((pos[1] & 0xFF, pos[1] >> 8)))
            cut[at:at + 2] = b"\x00\x00" if i % 12 == 4 else b"\xFF\xFF"
            cases.append((name + "-bad-offset", bytes(cut), len(plain)))
        else:
            cases.append((name, comp, len(plain) + k))
    return Batch(cases, dic)


def test_settings_give_the_same_results(env):
    lib, L, torch = env
    mixed = mixed_batch()
    kinds = {w[0] for w in mixed.want}
    assert "ok" in kinds and "OutputTooSmall" in kinds and len(kinds) >= 3, kinds
    one = real_batch("json", 65)
    ctxs = [("default", _ctx(lib)), ("decompress_shared_dict 0", _ctx(lib, decompress_shared_dict=0)), ("decompress_variant 1", _ctx(lib, decompress_variant=1))]
    try:
        for b, tag in ((one, "json-65"), (mixed, "mixed")):
            for mem in (L.MEM_DEVICE, L.MEM_HOST):
                res = []
                for name, ctx in ctxs:
                    r = b.run(env, ctx, mem)
                    b.check(r, None if mem == L.MEM_HOST else (False if name == "default" else True), "%s %s mem=%d" % (tag, name, mem))
                    res.append(r)
                same_results(res[0], res[1], b, tag + " shared_dict 0")
                same_results(res[0], res[2], b, tag + " variant 1")
    finally:
        for _, c in ctxs:
            lib.lz4flex_ctx_destroy(c)


# ---------------------------------------------------------------- 6. Python
def test_python_device_round_trip(env):
    lib, L, torch = env
    from lz4_flex_amd import block, workloads
    dev = torch.device("cuda", 0)
    n, rec = 2000, 4096
    src = workloads.log_lines(5000, n * rec // workloads.LINE + 1).reshape(-1)[:n * rec].contiguous().to(dev)
    dic = workloads.log_lines(0, 32768 // workloads.LINE + 1).reshape(-1)[:32768].contiguous().to(dev)
    in_off = torch.arange(n, dtype=torch.int64) * rec
    in_len = torch.full((n,), rec, dtype=torch.int64)
    comp, c_off, c_len, c_st = block.compress_blocks_with_shared_dict_device(src, in_off, in_len, dic)
    assert not bool(c_st.any())
    out, o_off, o_len, st = block.decompress_blocks_with_shared_dict_device(comp, c_off, c_len, dic)
    torch.cuda.synchronize()
    assert not bool(st.any())
    assert bool((o_len == rec).all()) and bool((o_off.cpu() == in_off).all())
    assert out.numel() == n * rec and torch.equal(out, src)
    # the blocks need their dictionary: without it they are not the input (or do not decode)
    h_comp, h_off, h_len = comp.cpu().numpy(), c_off.cpu().numpy(), c_len.cpu().numpy()
    assert reaches_dict([h_comp[int(h_off[i]):int(h_off[i]) + int(h_len[i])].tobytes() for i in range(0, n, 250)])


def test_python_host_against_per_block_dictionaries(env):
    lib, L, torch = env
    from lz4_flex_amd import block
    b = mixed_batch()
    dic = np.frombuffer(b.dic, dtype=np.uint8)
    o1, o2 = b.init.copy(), b.init.copy()
    l1, s1, d1 = block.decompress_batch_with_shared_dict(b.inb, b.in_off, b.in_len, dic, o1, b.out_off, b.cap)
    l2, s2, d2 = block.decompress_batch_with_dict(b.inb, b.in_off, b.in_len, dic, np.zeros(b.n, np.uint64), np.full(b.n, len(dic), np.uint32), o2,
                                                   b.out_off, b.cap)
    assert np.array_equal(l1, l2) and np.array_equal(s1, s2) and np.array_equal(d1, d2) and np.array_equal(o1, o2)
    b.check((o1, l1, s1, d1), None, "python host")


# ---------------------------------------------------------------- 7. the entry keeps no state
def test_two_calls_two_dictionaries_two_streams(env):
    lib, L, torch = env
    a, b = real_batch("json", 65), real_batch("log", 64)
    assert a.dic != b.dic
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ctx = _ctx(lib)
    try:
        fa = a.run(env, ctx, L.MEM_DEVICE, stream=s1.cuda_stream, sync=False)
        fb = b.run(env, ctx, L.MEM_DEVICE, stream=s2.cuda_stream, sync=False)
        fa2 = a.run(env, ctx, L.MEM_DEVICE, stream=s2.cuda_stream, sync=False)
        a.check(fa(), False, "first call")
        b.check(fb(), False, "second call")
        a.check(fa2(), False, "third call")
    finally:
        lib.lz4flex_ctx_destroy(ctx)
