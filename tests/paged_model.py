"""The paged rule of lz4flex_compress_paged (include/lz4flex_amd.h, lz4_paged.hip) as plain Python: n streams cut into pages of P bytes,
every page a self-contained LZ4 block that holds as much of its stream as fits -- the LZ4_compress_destSize loop, in rounds.  Test
infrastructure (a plain module, not a fixture): the GPU tests compare the library with run() over a round they compute with the entry
the loop is made of (lz4flex_compress_batch_fit), the CPU tests run it over the oracle's encoder and fit_model.fit.

A round is a callback `fit_round(windows, caps) -> [(out, used, status)]`: the result of lz4flex_compress_batch_fit for the n windows (bytes)
of this round at the n capacities; a stream that is not live has an empty window at capacity 0 whose result is ignored, so n is the same
in every round.  by_encoder() makes one from `encode_round(windows) -> [(block, status)]` and fit_model.fit."""
import fit_model as F

OK, E_OUTPUT_TOO_SMALL = 0, 1
PAGE_MIN, PAGE_MAX, WINDOW_LIMIT = 64, 4 << 20, 1 << 31


def lfit_page(page_size):
    """Lfit(P, infinity): what a page of literals alone holds"""
    return F.lfit(page_size, 1 << 62)


def windows_of(page_size, window_min=0, window_max=0):
    """(window_min, window_max) with the defaults resolved; None for arguments the entry refuses"""
    if not PAGE_MIN <= page_size <= PAGE_MAX:
        return None
    if window_min == 0:
        window_min = 4 * page_size
    if window_max == 0:
        window_max = max(window_min, 65536)
    return (window_min, window_max) if page_size <= window_min <= window_max <= WINDOW_LIMIT else None


def pages_bound(in_len, page_size):
    if not PAGE_MIN <= page_size <= PAGE_MAX:
        return 0
    L = lfit_page(page_size)
    return (in_len + L - 1) // L


def doublings(window_min, window_max):
    d = 0
    while window_min < window_max:
        window_min *= 2
        d += 1
    return d


def rounds_bound(max_in_len, page_size, window_min=0, window_max=0):
    w = windows_of(page_size, window_min, window_max)
    return 0 if w is None else pages_bound(max_in_len, page_size) + doublings(*w)


def by_encoder(encode_round):
    """the round of an encoder: its block for every window, cut to the capacity by the fit rule"""
    def fit_round(windows, caps):
        out = []
        for win, cap, (block, st) in zip(windows, caps, encode_round(windows)):
            if st != OK:
                out.append((b"", 0, st))
            else:
                out.append(F.fit(block, win, cap))
        return out
    return fit_round


class Paged:
    """What run() returns.  Per stream: n_pages, in_done, status, pages = [(page_src, block)] in order; rounds = the rounds in which a
    stream was live; offered = the window bytes handed to the encoder, retries included; retries per stream."""

    def __init__(self, n):
        self.n_pages, self.in_done, self.status = [0] * n, [0] * n, [OK] * n
        self.pages = [[] for _ in range(n)]
        self.retries = [0] * n
        self.rounds = self.offered = 0


def run(streams, page_size, capacity, fit_round, window_min=0, window_max=0, max_rounds=None):
    """the rule: streams = [bytes], capacity = [pages stream i may take]; max_rounds None = as many as it takes"""
    w = windows_of(page_size, window_min, window_max)
    if w is None:
        raise ValueError("page_size / window_min / window_max")
    window_min, window_max = w
    n = len(streams)
    r = Paged(n)
    W = [window_min] * n
    live = [len(s) != 0 for s in streams]
    for i in range(n):
        if live[i] and capacity[i] == 0:
            live[i], r.status[i] = False, E_OUTPUT_TOO_SMALL
    while any(live) and (max_rounds is None or r.rounds < max_rounds):
        r.rounds += 1
        at = list(r.in_done)
        windows = [bytes(s[at[i]:at[i] + min(W[i], len(s) - at[i])]) if live[i] else b"" for i, s in enumerate(streams)]
        caps = [page_size if live[i] else 0 for i in range(n)]
        r.offered += sum(len(x) for x in windows)
        results = fit_round(windows, caps)
        assert len(results) == n
        for i, (out, used, st) in enumerate(results):
            if not live[i]:
                continue
            offered, left = len(windows[i]), len(streams[i]) - at[i]
            if st != OK:
                live[i], r.status[i] = False, st
            elif used == offered and offered < left and W[i] < window_max:
                W[i] = min(2 * W[i], window_max)
                r.retries[i] += 1
            else:
                r.pages[i].append((at[i], bytes(out)))
                r.in_done[i] += used
                r.n_pages[i] += 1
                if r.in_done[i] == len(streams[i]):
                    live[i] = False
                elif r.n_pages[i] == capacity[i]:
                    live[i], r.status[i] = False, E_OUTPUT_TOO_SMALL
    for i in range(n):
        if live[i]:
            r.status[i] = E_OUTPUT_TOO_SMALL
    return r


def replay_offered(in_len, page_src, in_done, page_size, window_min=0, window_max=0):
    """the window bytes one stream was offered, from its results alone (the commits of a finished stream): a commit at `pos` that used
    `used` bytes was offered min(W, left) bytes, after a retry at every W that `used` reaches or outgrows (such a window fit whole with
    more behind it; exact as long as a longer window never commits fewer bytes than a shorter one that fit whole)"""
    window_min, window_max = windows_of(page_size, window_min, window_max)
    W, total = window_min, 0
    ends = list(page_src[1:]) + [in_done]
    for pos, end in zip(page_src, ends):
        left, used = in_len - pos, end - pos
        while True:
            w = min(W, left)
            total += w
            if used >= w and w < left and W < window_max:
                W = min(2 * W, window_max)
                continue
            break
    return total
