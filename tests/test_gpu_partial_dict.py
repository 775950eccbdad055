"""GPU (-m gpu): lz4flex_decompress_batch_partial_shared_dict / _dict_set / lz4flex_decompress_partial_into_with_dict -- the first
target[i] bytes of every block of a batch that was compressed against a dictionary, by the sequence decoder's form with a dictionary
and a target (lz4_decompress_seq.hip Dec<G, true, true>) and by the reference-order form behind it (lz4_decompress.hip
decode_block<16, true, true>).

Checker: tests/partial_dict_model.py (the contract in Python, pinned to the oracle by tests/test_partial_dict_model.py) for status,
out_len and bytes.  Every sink is exactly `target` bytes between canaries at an out_off that is no multiple of 16: a byte stored at or
behind out_off + target, or in front of out_off, fails the test.  The dictionary lies between canaries too and is compared with its
copy after every call, as is the input buffer."""
import ctypes as C

import numpy as np
import pytest

import partial_dict_model as D
import partial_model as M

pytestmark = pytest.mark.gpu
REDO = 0x7F000001
INVALID = 64
NO_DICT = 0xFFFFFFFF
CANARY = 64
FILL = 0xA5
DICT_AT = CANARY + 3          # where a dictionary starts in its buffer: no multiple of 16


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


def _set(lib, dicts):
    """a lz4flex_dict_set of the dictionaries (host memory)"""
    lens = np.array([len(d) for d in dicts], dtype=np.uint32)
    offs = (np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint64)
    flat = np.frombuffer(b"".join(dicts) + b"\0", dtype=np.uint8).copy()
    h = C.c_void_p()
    rc = lib.lz4flex_dict_set_create(None, C.c_void_p(flat.ctypes.data), C.c_void_p(offs.ctypes.data), C.c_void_p(lens.ctypes.data), len(dicts), 0,
                                     C.byref(h))
    assert rc == 0 and h.value, rc
    return h


class Batch:
    """entries: (name, block, target); want: the model's (status, bytes) per entry.  Sink i: CANARY bytes of FILL, target bytes, CANARY
    bytes of FILL, at an out_off that is no multiple of 16; the blocks lie back to back from byte 3 of the input buffer.  An entry
    (name, block, target, room) has a sink of `room` bytes instead: targets no buffer holds, for blocks that end long before them
    (MEM_DEVICE only: a host call stages what the targets say)."""

    def __init__(self, entries, want, ids=None):
        self.entries, self.want, self.n = entries, want, len(entries)
        comps = [e[1] for e in entries]
        self.in_len = np.array([len(c) for c in comps], dtype=np.uint32)
        self.in_off = (np.concatenate([[0], np.cumsum(self.in_len[:-1], dtype=np.uint64)]) + 3).astype(np.uint64)
        self.inb = np.frombuffer(bytes(3) + b"".join(comps) + bytes(64), dtype=np.uint8).copy()
        self.target = np.array([e[2] for e in entries], dtype=np.uint32)
        self.ids = None if ids is None else np.array(ids, dtype=np.uint32)
        self.room = [e[3] if len(e) > 3 else e[2] for e in entries]
        off, o = [], 0
        for room in self.room:
            o += CANARY
            if o % 16 == 0:
                o += 5
            off.append(o)
            o += room + CANARY
        self.out_off = np.array(off, dtype=np.uint64)
        self.size = o + 64

    def sub(self, idx):
        idx = list(idx)
        return Batch([self.entries[i] for i in idx], [self.want[i] for i in idx], None if self.ids is None else self.ids[idx])

    def run(self, env, ctx, mem, how="shared", dic=None, dict_set=None):
        """how: "shared" / "set": the new entries; "partial": lz4flex_decompress_batch_partial; "full": lz4flex_decompress_batch_shared_dict
        with the targets as capacities.  Returns (out, out_len, status)."""
        lib, L, torch = env
        n = self.n
        out = np.full(self.size, FILL, dtype=np.uint8)
        dbuf = np.frombuffer(bytes([FILL]) * DICT_AT + (dic or b"") + bytes([FILL]) * CANARY, dtype=np.uint8).copy()
        arrays = dict(inb=self.inb.copy(), in_off=self.in_off, in_len=self.in_len, out=out, out_off=self.out_off, target=self.target,
                      out_len=np.full(n, 0xDEADBEEF, dtype=np.uint32), status=np.full(n, -1, dtype=np.int32), dbuf=dbuf.copy(),
                      ids=self.ids if self.ids is not None else np.zeros(n, dtype=np.uint32))
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
        dp, dn = (C.c_void_p(addr["dbuf"] + DICT_AT), len(dic)) if dic else (None, 0)
        head = (ctx, p["inb"], p["in_off"], p["in_len"], n)
        if how == "shared":
            rc = lib.lz4flex_decompress_batch_partial_shared_dict(*head, p["out"], p["out_off"], p["target"], p["out_len"], p["status"], dp, dn, mem, sp)
        elif how == "set":
            rc = lib.lz4flex_decompress_batch_partial_dict_set(*head, p["ids"], p["out"], p["out_off"], p["target"], p["out_len"], p["status"],
                                                               dict_set, mem, sp)
        elif how == "partial":
            rc = lib.lz4flex_decompress_batch_partial(*head, p["out"], p["out_off"], p["target"], p["out_len"], p["status"], mem, sp)
        else:
            rc = lib.lz4flex_decompress_batch_shared_dict(*head, p["out"], p["out_off"], p["target"], p["out_len"], p["status"], None, dp, dn, mem, sp)
        assert rc == 0, (how, rc, L.last_error())
        if not host:
            torch.cuda.synchronize()
            for k in ("inb", "out", "out_len", "status", "dbuf"):
                arrays[k].view(np.uint8).reshape(-1)[:] = keep[k].cpu().numpy()
        assert np.array_equal(arrays["inb"], self.inb), "the input buffer was written"
        assert np.array_equal(arrays["dbuf"], dbuf), "the dictionary or its canaries were written"
        return out, arrays["out_len"], arrays["status"]

    def check(self, res, what, marked_ok=False):
        """status and out_len are the model's, the first out_len bytes of a sink too, and every byte outside the sinks is untouched (what
        a sink holds behind out_len, or after an error, is not specified -- but a refused id leaves its sink alone).  marked_ok
        ("decompress_second_pass" 0): a block may instead be left marked with out_len 0.  Returns the marked blocks."""
        out, out_len, status = res
        exp = np.full(self.size, FILL, dtype=np.uint8)
        care = np.ones(self.size, dtype=bool)
        marked = []
        for i in range(self.n):
            name, (wst, wbytes) = self.entries[i][0], self.want[i]
            st, ol, o, t = int(status[i]), int(out_len[i]), int(self.out_off[i]), int(self.target[i])
            if wst != INVALID:
                care[o:o + self.room[i]] = False
            if marked_ok and st == REDO and wst != INVALID:
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


def same_results(a, b, batch, what):
    """two runs of one batch: status and out_len equal, and the first out_len bytes of every sink"""
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[1], b[1]), what
    for i in range(batch.n):
        o, ol = int(batch.out_off[i]), int(a[1][i])
        assert np.array_equal(a[0][o:o + ol], b[0][o:o + ol]), (what, batch.entries[i][0], int(batch.target[i]))


MODES = [("device", 1), ("device", 0), ("host", 1), ("host", 0)]


def _mem(env, where):
    return env[1].MEM_DEVICE if where == "device" else env[1].MEM_HOST


# ---------------------------------------------------------------- the sets, built once
_sets = {}


def dict_set_of(n):
    """(dictionary, Batch of every block of dict_cases / damaged_cases at each of its targets, valid flags, per-entry 'damaged' flags)"""
    if n not in _sets:
        dic = D.dictionary(n)
        entries, want, valid = [], [], []
        for name, c, _plain, targets in D.dict_cases(dic):
            prof = D.Profile(c, dic)
            for t in targets:
                entries.append((name, c, t))
                want.append(prof.at(t))
                valid.append(prof.status == 0)
        for name, c, targets in D.damaged_cases(dic):
            prof = D.Profile(c, dic)
            for t in targets:
                entries.append((name, c, t))
                want.append(prof.at(t))
                valid.append(False)
        _sets[n] = (dic, Batch(entries, want), valid)
    return _sets[n]


def plain_set_against(dic):
    """partial_model's hand-written sets, unchanged, with the model's word on what they are against `dic`"""
    key = ("plain", len(dic))
    if key not in _sets:
        entries, want = [], []
        for name, c, _plain, targets in M.writer_cases():
            prof = D.Profile(c, dic)
            for t in targets:
                entries.append((name, c, t))
                want.append(prof.at(t))
        for name, c, targets in M.corrupted_cases():
            prof = D.Profile(c, dic)
            for t in targets:
                entries.append((name, c, t))
                want.append(prof.at(t))
        _sets[key] = Batch(entries, want)
    return _sets[key]


# ---------------------------------------------------------------- 1. the dictionary-specific cases
@pytest.mark.parametrize("where,partial", MODES)
@pytest.mark.parametrize("n", D.DICT_LENGTHS)
def test_dictionary_cases(env, n, where, partial):
    lib = env[0]
    dic, batch, _ = dict_set_of(n)
    assert batch.n < 3000 and 0 in {w[0] for w in batch.want} and 4 in {w[0] for w in batch.want}
    ctx = _ctx(lib, decompress_partial=partial)
    try:
        batch.check(batch.run(env, ctx, _mem(env, where), dic=dic), "%d bytes of dictionary, %s, decompress_partial %d" % (n, where, partial))
    finally:
        lib.lz4flex_ctx_destroy(ctx)


@pytest.mark.parametrize("setting", ["decompress_variant", "decompress_shared_dict"])
def test_the_settings_that_select_the_reference_order(env, setting):
    """"decompress_variant" 1 and "decompress_shared_dict" 0 send every block through the reference-order kernel, as "decompress_partial" 0 does"""
    lib, L, _ = env
    dic, batch, _ = dict_set_of(1281)
    ctx = _ctx(lib, **{setting: 1 if setting == "decompress_variant" else 0, "decompress_second_pass": 0})
    try:
        res = batch.run(env, ctx, L.MEM_DEVICE, dic=dic)
        assert REDO not in set(int(s) for s in res[2])          # (nothing was handed back: no first pass ran)
        batch.check(res, setting)
    finally:
        lib.lz4flex_ctx_destroy(ctx)


# ---------------------------------------------------------------- 2. the plain partial sets against a dictionary
@pytest.mark.parametrize("where,partial", MODES)
@pytest.mark.parametrize("n", [17, 70001])
def test_plain_sets_against_a_dictionary(env, n, where, partial):
    """blocks that never reach into their dictionary give the plain partial results; an offset one past the output is the model's to judge"""
    lib = env[0]
    dic = D.dictionary(n)
    batch = plain_set_against(dic)
    assert batch.n > 600 and {w[0] for w in batch.want} >= {0, 2, 3, 4}
    ctx = _ctx(lib, decompress_partial=partial)
    try:
        batch.check(batch.run(env, ctx, _mem(env, where), dic=dic), "%d bytes of dictionary, %s, decompress_partial %d" % (n, where, partial))
    finally:
        lib.lz4flex_ctx_destroy(ctx)


# ---------------------------------------------------------------- 3. the equalities
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("n", [17, 1281, 70001])
def test_a_set_of_one_is_the_shared_entry(env, n, where):
    lib = env[0]
    dic, batch, _ = dict_set_of(n)
    ctx, h = _ctx(lib), _set(lib, [dic])
    try:
        shared = batch.run(env, ctx, _mem(env, where), dic=dic)
        one = batch.run(env, ctx, _mem(env, where), "set", dict_set=h)
        batch.check(one, "a set of one")
        same_results(shared, one, batch, "shared against a set of one")
    finally:
        lib.lz4flex_dict_set_free(h)
        lib.lz4flex_ctx_destroy(ctx)


@pytest.mark.parametrize("where", ["device", "host"])
def test_no_dictionary_is_the_plain_partial_entry(env, where):
    """dict NULL, dict_len 0, an id of 0xFFFFFFFF and an id whose dictionary is empty"""
    lib = env[0]
    batch = plain_set_against(b"")
    ctx, h = _ctx(lib), _set(lib, [b"", D.dictionary(17)])
    try:
        mem = _mem(env, where)
        plain = batch.run(env, ctx, mem, "partial")
        batch.check(plain, "the plain partial entry")
        same_results(plain, batch.run(env, ctx, mem, "shared", dic=None), batch, "dict NULL")
        for ids in (np.full(batch.n, NO_DICT, dtype=np.uint32), np.zeros(batch.n, dtype=np.uint32)):
            b = Batch(batch.entries, batch.want, ids)
            res = b.run(env, ctx, mem, "set", dict_set=h)
            b.check(res, "ids %#x" % int(ids[0]))
            same_results(plain, res, batch, "ids %#x" % int(ids[0]))
    finally:
        lib.lz4flex_dict_set_free(h)
        lib.lz4flex_ctx_destroy(ctx)


@pytest.mark.parametrize("n", [17, 1281, 70001])
def test_a_target_beyond_the_size_is_the_full_entry(env, n):
    """target >= size on the valid cases: lz4flex_decompress_batch_shared_dict with out_cap = target"""
    lib, L, _ = env
    dic, batch, valid = dict_set_of(n)
    blocks = {}
    for (name, c, _t), ok in zip(batch.entries, valid):
        if ok:
            blocks.setdefault(c, name)
    entries, want = [], []
    for c, name in blocks.items():
        plain = D.partial_with_dict(c, M.FOREVER, dic)
        for t in (len(plain[1]), len(plain[1]) + 1, len(plain[1]) + 300):
            entries.append((name, c, t))
            want.append(plain)
    b = Batch(entries, want)
    ctx = _ctx(lib)
    try:
        for mem in (L.MEM_DEVICE, L.MEM_HOST):
            new, full = b.run(env, ctx, mem, dic=dic), b.run(env, ctx, mem, "full", dic=dic)
            b.check(new, "target >= size")
            b.check(full, "the full entry")
            same_results(new, full, b, "target >= size against the full entry")
    finally:
        lib.lz4flex_ctx_destroy(ctx)


# ---------------------------------------------------------------- 4. a set of four
def _mixed():
    """K = 4 (0, 17, 1 281 and 70 001 bytes), ids cycling over 0 .. 3 and 0xFFFFFFFF -- each block with the dictionary it was written
    against, the plain blocks with id 0 or none -- and two blocks with ids the set does not have"""
    if "mixed" not in _sets:
        lens = [0, 17, 1281, 70001]
        dicts = [D.dictionary(n) if n else b"" for n in lens]
        pools = []
        plain = plain_set_against(b"")
        for k, n in enumerate(lens):
            b = dict_set_of(n)[1] if n else plain
            pools.append([(e, w) for e, w in zip(b.entries, b.want)][k::7])
        pools.append([(e, w) for e, w in zip(plain.entries, plain.want)][3::7])
        entries, want, ids = [], [], []
        for row in zip(*pools):
            for k, (e, w) in enumerate(row):
                entries.append(e)
                want.append(w)
                ids.append(k if k < 4 else NO_DICT)
        for at, bad in ((11, 4), (len(entries) - 7, 0x7FFFFFFF)):
            name, c, t = entries[at]
            entries[at], want[at], ids[at] = (name + " with an id the set does not have", c, max(t, 40)), (INVALID, b""), bad
        _sets["mixed"] = (dicts, Batch(entries, want, ids))
    return _sets["mixed"]


@pytest.mark.parametrize("where,partial", MODES)
def test_a_set_of_four(env, where, partial):
    lib = env[0]
    dicts, batch = _mixed()
    assert 300 < batch.n < 3000 and set(batch.ids.tolist()) == {0, 1, 2, 3, NO_DICT, 4, 0x7FFFFFFF}
    assert {w[0] for w in batch.want} >= {0, 3, 4, 5, INVALID}
    ctx, other, h = _ctx(lib, decompress_partial=partial), _ctx(lib, decompress_partial=partial), _set(lib, dicts)
    try:
        batch.check(batch.run(env, ctx, _mem(env, where), "set", dict_set=h), "%s, decompress_partial %d" % (where, partial))
        batch.check(batch.run(env, other, _mem(env, where), "set", dict_set=h), "a second context, the same set")
    finally:
        lib.lz4flex_dict_set_free(h)
        lib.lz4flex_ctx_destroy(ctx)
        lib.lz4flex_ctx_destroy(other)


# ---------------------------------------------------------------- 5. batch sizes
@pytest.mark.parametrize("where", ["device", "host"])
def test_batch_sizes(env, where):
    """1 block, 65 blocks (two workgroups of the reference-order kernel and a ragged one); the whole set in one call is test 1"""
    lib = env[0]
    dic, batch, _ = dict_set_of(1281)
    h = _set(lib, [dic])
    ctx, ref = _ctx(lib), _ctx(lib, decompress_partial=0)
    try:
        for idx in ([137], range(100, 165), range(batch.n - 65, batch.n)):
            b = batch.sub(idx)
            for c, what in ((ctx, ""), (ref, ", decompress_partial 0")):
                b.check(b.run(env, c, _mem(env, where), dic=dic), "%s, %d blocks%s" % (where, b.n, what))
                b.check(b.run(env, c, _mem(env, where), "set", dict_set=h), "%s, %d blocks, a set%s" % (where, b.n, what))
    finally:
        lib.lz4flex_dict_set_free(h)
        lib.lz4flex_ctx_destroy(ctx)
        lib.lz4flex_ctx_destroy(ref)


# ---------------------------------------------------------------- 6. the kernel, not the fallback
@pytest.mark.parametrize("n", D.DICT_LENGTHS)
def test_the_sequence_decoder_decodes_what_it_decodes_in_full(env, n):
    """"decompress_second_pass" 0: a block the new form hands back stays marked.  At no target may it mark a block that the full
    dictionary form (lz4flex_decompress_batch_shared_dict, the same setting, the block's full size, the same run) does not mark; and every
    damaged block whose error lies in front of the stop stays marked with out_len 0."""
    lib, L, _ = env
    dic, batch, valid = dict_set_of(n)
    blocks = {}
    for (name, c, _t), ok in zip(batch.entries, valid):
        if ok:
            blocks.setdefault(c, name)
    full = Batch([(name, c, len(D.Profile(c, dic).out)) for c, name in blocks.items()], [D.partial_with_dict(c, M.FOREVER, dic) for c in blocks])
    ctx = _ctx(lib, decompress_second_pass=0)
    try:
        marked = full.check(full.run(env, ctx, L.MEM_DEVICE, "full", dic=dic), "the full dictionary form", marked_ok=True)
        full_marked = {full.entries[i][1] for i in marked}
        assert len(full_marked) < len(blocks) // 4, sorted(blocks[c] for c in full_marked)[:10]      # (the comparison below says something)
        got = batch.check(batch.run(env, ctx, L.MEM_DEVICE, dic=dic), "every target", marked_ok=True)
        extra = [(batch.entries[i][0], batch.entries[i][2]) for i in got if valid[i] and batch.entries[i][1] not in full_marked]
        assert not extra, extra[:10]
        errors = [i for i, w in enumerate(batch.want) if w[0] != 0]
        assert len(errors) > 20 and set(errors) <= set(got), [(batch.entries[i][0], batch.entries[i][2]) for i in set(errors) - set(got)][:10]
    finally:
        lib.lz4flex_ctx_destroy(ctx)


def test_targets_the_position_space_does_not_hold(env):
    """The sequence decoder counts positions from the dictionary's start and keeps them below 4 GiB - 64 KiB.  A target beyond what is
    left of that space must not be cut to it (the decode would stop early with status 0) and must not cost a valid block its first
    pass either: with "decompress_second_pass" 0 a valid block decodes to its end, unmarked, unless the full dictionary form hands it
    back too at that capacity; the damaged blocks and those that end in a match are handed back (their errors with the second pass on)."""
    lib, L, _ = env
    limit = 0xFFFF0000
    for n in (17, 70001):
        dic, batch, _ = dict_set_of(n)
        pv = (min(n, 65536) + 15) & ~15
        blocks = {}
        for name, c, _t in batch.entries[::9]:
            blocks.setdefault(c, name)
        entries, want = [], []
        for c, name in blocks.items():
            prof = D.Profile(c, dic)
            for t in (limit - pv - 1, limit - pv, limit - pv + 1, limit, 0xFFFFFFFF):
                # (after an error the sink's target bytes may hold anything: the reference-order kernel's 8-byte literal store reaches a
                # few bytes behind where the error is met, so a damaged block gets room for that; a valid block gets its size and a byte)
                entries.append((name, c, t, len(prof.out) + (1 if prof.status == 0 else 64)))
                want.append(prof.at(t))
        b = Batch(entries, want)
        assert {w[0] for w in b.want} >= {0, 3, 4}
        ctx, first = _ctx(lib), _ctx(lib, decompress_second_pass=0)
        try:
            b.check(b.run(env, ctx, L.MEM_DEVICE, dic=dic), "%d bytes of dictionary" % n)
            marked = b.check(b.run(env, first, L.MEM_DEVICE, dic=dic), "%d bytes of dictionary, the first pass" % n, marked_ok=True)
            full = b.check(b.run(env, first, L.MEM_DEVICE, "full", dic=dic), "%d bytes of dictionary, the full form's first pass" % n, marked_ok=True)
            errors = {i for i, w in enumerate(b.want) if w[0] != 0}
            assert errors <= set(marked) and set(marked) - errors <= set(full), (n, sorted(set(marked) - errors - set(full))[:10])
            assert len(set(marked) - errors) < (b.n - len(errors)) // 4          # (the first pass decodes: the comparison says something)
        finally:
            lib.lz4flex_ctx_destroy(ctx)
            lib.lz4flex_ctx_destroy(first)


# ---------------------------------------------------------------- 7. the Python layer
def test_python_layer(env):
    """the five functions give the ctypes calls' results on 65 blocks; the scalar one returns the bytes or raises the model's error class"""
    lib, L, torch = env
    from lz4_flex_amd import block
    dic, batch, _ = dict_set_of(4096)
    idx = []
    for code in (3, 4, 5):
        idx += [i for i, w in enumerate(batch.want) if w[0] == code][:6]
    good = [i for i, w in enumerate(batch.want) if w[0] == 0]
    idx += good[::len(good) // (65 - len(idx)) + 1]
    idx += [i for i in good if i not in idx][:65 - len(idx)]
    b = batch.sub(sorted(idx))
    assert b.n == 65 and {w[0] for w in b.want} == {0, 3, 4, 5}
    ref = b.run(env, None, L.MEM_HOST, dic=dic)
    b.check(ref, "ctypes")
    darr = np.frombuffer(dic, dtype=np.uint8)
    out = np.full(b.size, FILL, dtype=np.uint8)
    out_len, status = block.decompress_batch_partial_with_shared_dict(b.inb, b.in_off, b.in_len, darr, out, b.out_off, b.target)
    b.check((out, out_len, status), "decompress_batch_partial_with_shared_dict")
    ids = np.ones(b.n, dtype=np.uint32)
    dev = torch.device("cuda", 0)
    t_in, t_off, t_len, t_tgt = (torch.from_numpy(b.inb).to(dev), torch.from_numpy(b.in_off.astype(np.int64)), torch.from_numpy(b.in_len.astype(np.int64)),
                                 torch.from_numpy(b.target.astype(np.int64)))
    with block.DictSet([b"", dic]) as ds:
        out = np.full(b.size, FILL, dtype=np.uint8)
        out_len, status = block.decompress_batch_partial_with_dict_set(b.inb, b.in_off, b.in_len, ids, ds, out, b.out_off, b.target)
        b.check((out, out_len, status), "decompress_batch_partial_with_dict_set")
        packed = [block.decompress_blocks_partial_with_shared_dict_device(t_in, t_off, t_len, t_tgt, torch.from_numpy(darr.copy()).to(dev)),
                  block.decompress_blocks_partial_with_dict_set_device(t_in, t_off, t_len, t_tgt, torch.from_numpy(ids.astype(np.int64)), ds)]
        torch.cuda.synchronize()
    for d_out, d_off, d_len, d_st in packed:
        flat, off = d_out.cpu().numpy(), d_off.cpu().numpy()
        assert flat.size == int(b.target.sum()) and np.array_equal(off, np.cumsum(b.target.astype(np.int64)) - b.target)
        assert np.array_equal(d_len.cpu().numpy().astype(np.uint32), ref[1]) and np.array_equal(d_st.cpu().numpy(), ref[2])
        for i, (st, want) in enumerate(b.want):
            if st == 0:
                assert bytes(flat[int(off[i]):int(off[i]) + len(want)]) == want, b.entries[i][0]
    errors = {3: block.ExpectedAnotherByte, 4: block.OffsetZero, 5: block.OffsetOutOfBounds}
    raised = set()
    for (name, c, t), (st, want) in zip(b.entries, b.want):
        if st == 0:
            assert block.decompress_partial_with_dict(c, t, dic) == want, (name, t)
        else:
            with pytest.raises(errors[st]):
                block.decompress_partial_with_dict(c, t, dic)
            raised.add(st)
    assert raised == {3, 4, 5}, raised
    assert block.decompress_partial_with_dict(b"\x50hello", 3, b"") == b"hel"
