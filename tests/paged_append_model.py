"""The rule of lz4flex_paged_append (include/lz4flex_amd.h, lz4_paged_append.hip, paged_append.h) as plain Python: new bytes for any
subset of n paged streams, the tail page of every such stream reopened and the paged rule of lz4flex_compress_paged resumed over
tail ++ add.  Test infrastructure (a plain module, not a fixture): the CPU tests run it over the oracle's encoder and fit_model.fit, and
hold paged_append.h (compiled for the host, tests/sim/paged_append_shim.cpp) to its steps 1 to 4.

The rounds are paged_model.run -- the rule is resumed unchanged, so the model calls it and does not restate it -- over the streams V_i,
empty for a dead stream; a round is paged_model's callback `fit_round(windows, caps)`.  The reopen is a callback
`decode_partial(block, target) -> (status, bytes)`: lz4flex_decompress_batch_partial for one page."""
import paged_model as M

OK, E_OUTPUT_TOO_SMALL, E_EXPECTED_ANOTHER_BYTE, E_INVALID_ARG = 0, 1, 3, 64
NO_STAGE = (1 << 64) - 1
U32_MAX = 0xFFFFFFFF
STAGE_ALIGN = 64
GO = None                                  # the `pre` of a stream that goes on to the reopen


class Tables:
    """Paged streams as the header's arrays (lists of ints) and the page file as {entry: the page's first page_len bytes}; entries are
    absolute, page_off[0] need not be 0.  run() updates it in place."""

    def __init__(self, page_size, page_off, page_len, page_src, n_pages, in_done, blocks=None):
        self.page_size, self.page_off, self.page_len, self.page_src = page_size, list(page_off), list(page_len), list(page_src)
        self.n_pages, self.in_done = list(n_pages), list(in_done)
        self.blocks = dict(blocks or {})
        self.n = len(self.n_pages)

    def copy(self):
        return Tables(self.page_size, self.page_off, self.page_len, self.page_src, self.n_pages, self.in_done, self.blocks)

    def pages_of(self, i):
        """[(page_src, block)] of stream i, as paged_model.Paged.pages holds them"""
        first = self.page_off[i]
        return [(self.page_src[e], self.blocks[e]) for e in range(first, first + self.n_pages[i])]


def empty_tables(page_size, capacity, first=0):
    """n fresh streams with room for capacity[i] pages each"""
    page_off = [first]
    for c in capacity:
        page_off.append(page_off[-1] + c)
    entries = page_off[-1]
    return Tables(page_size, page_off, [0] * entries, [0] * entries, [0] * len(capacity), [0] * len(capacity))


class Rec:
    """one stream, located: steps 1 to 3"""
    __slots__ = ("first", "C", "k", "S", "A", "base", "T", "idle", "bad")


def locate(t, i, A, window_max):
    r = Rec()
    first, nxt = t.page_off[i], t.page_off[i + 1]
    r.first, r.C, r.k, r.S, r.A, r.base, r.T = first, max(nxt - first, 0), t.n_pages[i], t.in_done[i], A, 0, 0
    r.idle, r.bad = A == 0, False
    if r.idle:
        return r
    r.bad = True
    if nxt < first or r.k > r.C or r.S + A > U32_MAX:
        return r
    if r.k == 0:
        r.bad = r.S != 0
        return r
    e = first + r.k - 1
    if t.page_len[e] == 0 or t.page_len[e] > t.page_size or t.page_src[e] >= r.S or r.S - t.page_src[e] > window_max:
        return r
    r.base, r.T, r.bad = t.page_src[e], r.S - t.page_src[e], False
    return r


def slot_bytes(r):
    return 0 if r.idle or r.bad else (r.T + r.A + STAGE_ALIGN - 1) // STAGE_ALIGN * STAGE_ALIGN


def k0_of(r):
    return r.k - 1 if r.k else 0


def stage_bound(sum_add_len, n, window_max=0):
    window_max = window_max or 65536
    return sum_add_len + n * (window_max + 63) if 64 <= window_max <= 1 << 31 else 0


class Plan:
    """steps 1 to 4 of a call: recs, pre (GO, or the status the stream has before a page is decoded), slot (the exclusive sums, n + 1),
    stage_off, tail_src"""


def plan(t, add_len, window_max, stage_cap=None):
    p = Plan()
    p.recs = [locate(t, i, A, window_max) for i, A in enumerate(add_len)]
    p.slot, p.pre, p.stage_off, p.tail_src = [0], [], [], []
    for r in p.recs:
        at = p.slot[-1]
        need = slot_bytes(r)
        p.slot.append(at + need)
        if r.idle:
            pre = OK
        elif r.bad:
            pre = E_INVALID_ARG
        else:
            pre = GO if stage_cap is None or at + need <= stage_cap else E_OUTPUT_TOO_SMALL
        p.pre.append(pre)
        p.stage_off.append(at if pre is GO else NO_STAGE)
        p.tail_src.append(r.S if r.idle or r.bad else r.base)
    return p


class Appended:
    """What run() returns.  status, stage_off, tail_src per stream; stage = {i: V_i} for the streams that were reopened; plan = the Plan;
    rounds = paged_model.Paged of the resumed rounds (None when no stream went on)."""


def run(t, adds, fit_round, decode_partial, window_min=0, window_max=0, max_rounds=None, stage_cap=None):
    """the rule: t is updated in place"""
    w = M.windows_of(t.page_size, window_min, window_max)
    if w is None:
        raise ValueError("page_size / window_min / window_max")
    window_min, window_max = w
    n = t.n
    assert len(adds) == n
    p = plan(t, [len(a) for a in adds], window_max, stage_cap)
    res = Appended()
    res.plan, res.status, res.stage_off, res.tail_src, res.stage, res.rounds = p, [OK] * n, p.stage_off, p.tail_src, {}, None
    V, cap = [b""] * n, [0] * n
    for i, (r, pre) in enumerate(zip(p.recs, p.pre)):
        if pre is not GO:
            res.status[i] = pre
            continue
        tail = b""
        if r.T:
            e = r.first + r.k - 1
            st, tail = decode_partial(t.blocks[e][:t.page_len[e]], r.T)
            if st != OK or len(tail) < r.T:
                res.status[i] = st if st != OK else E_EXPECTED_ANOTHER_BYTE
                continue
        V[i], cap[i] = bytes(tail) + bytes(adds[i]), r.C - k0_of(r)
        res.stage[i] = V[i]
    if not res.stage:
        return res
    res.rounds = M.run(V, t.page_size, cap, fit_round, window_min, window_max, max_rounds)
    for i in res.stage:
        r, k0 = p.recs[i], k0_of(p.recs[i])
        for j, (pos, block) in enumerate(res.rounds.pages[i]):
            e = r.first + k0 + j
            t.page_len[e], t.page_src[e], t.blocks[e] = len(block), r.base + pos, block
        t.n_pages[i], t.in_done[i], res.status[i] = k0 + res.rounds.n_pages[i], r.base + res.rounds.in_done[i], res.rounds.status[i]
    return res
