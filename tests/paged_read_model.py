"""The rule of lz4flex_paged_read_ranges (include/lz4flex_amd.h, lz4_paged_read.hip, paged_range.h) as plain Python: where bytes
[off, off + len) of stream i lie in the page table lz4flex_compress_paged wrote, which touched page is a head, what every touched page's
decode item is, who is served by max_items / scratch_cap, and the status a range gets before (and, given the pages' decode results,
after) the decoders ran.  Test infrastructure (a plain module, not a fixture): the CPU tests compare it with a brute-force byte-to-page
map and with paged_range.h compiled for the host, the GPU tests take every expected out_len / status from it -- the expected BYTES are
the source's own.

The tables may hold anything: like the C++ it never indexes outside the stream's entries [first, first + C)."""
import fit_model as F

OK, E_OUTPUT_TOO_SMALL, E_EXPECTED_ANOTHER_BYTE, E_INVALID_ARG = 0, 1, 3, 64
PAGE_MIN, PAGE_MAX, HEAD_ALIGN = 64, 4 << 20, 64
WHOLE = 0xFFFFFFFF


class Tables:
    """what lz4flex_compress_paged produced: page_off (n + 1, entries), page_len / page_src per entry, n_pages / in_done per stream"""

    def __init__(self, page_size, page_off, page_len, page_src, n_pages, in_done):
        self.page_size = int(page_size)
        self.page_off, self.page_len, self.page_src = [int(v) for v in page_off], [int(v) for v in page_len], [int(v) for v in page_src]
        self.n_pages, self.in_done = [int(v) for v in n_pages], [int(v) for v in in_done]
        self.n = len(self.n_pages)


def tables_of(paged, page_size, capacity, first=0):
    """the tables of a paged_model.run result laid out as the entry lays them out: stream i owns capacity[i] entries from first on;
    entries nobody committed hold 0.  Returns (Tables, pages) with pages = {entry: block}."""
    page_off = [first]
    for c in capacity:
        page_off.append(page_off[-1] + c)
    page_len, page_src, blocks = [0] * page_off[-1], [0] * page_off[-1], {}
    for i, pages in enumerate(paged.pages):
        for j, (pos, block) in enumerate(pages):
            e = page_off[i] + j
            page_len[e], page_src[e], blocks[e] = len(block), pos, block
    return Tables(page_size, page_off, page_len, page_src, paged.n_pages, paged.in_done), blocks


def lfit_page(page_size):
    return F.lfit(page_size, 1 << 62)


def pages_bound(length, page_size):
    """the pages a range of `length` bytes can touch in a table lz4flex_compress_paged wrote; 0 for a page size it refuses"""
    if not PAGE_MIN <= page_size <= PAGE_MAX:
        return 0
    if length < 2:
        return length
    return 2 + (length - 2) // lfit_page(page_size)


def clip_len(off, length, S):
    return 0 if off >= S else min(length, S - off)


def page_of(src, pos):
    """the last j < len(src) with src[j] <= pos, by the C++'s binary search (so that a table that does not ascend gives the same j)"""
    lo, hi = 0, len(src)
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if src[mid] <= pos:
            lo = mid
        else:
            hi = mid
    return lo


class Rec:
    """one located range: stream, off, len (clipped), first, k, S, j0, nb, head, head_bytes, bad, no_stream"""

    def __init__(self, stream, off):
        self.stream, self.off, self.len = stream, off, 0
        self.first = self.k = self.S = self.j0 = self.nb = self.head_bytes = 0
        self.head = self.bad = self.no_stream = False

    @property
    def head_slot(self):
        return (self.head_bytes + HEAD_ALIGN - 1) // HEAD_ALIGN * HEAD_ALIGN


def locate(t, i, off, length):
    r = Rec(i, off)
    if i >= t.n:
        r.no_stream = True
        return r
    first = t.page_off[i]
    C = max(t.page_off[i + 1] - first, 0)
    r.first, r.k, r.S = first, min(t.n_pages[i], C), t.in_done[i]
    r.len = clip_len(off, length, r.S)
    if r.len == 0:
        return r
    if r.k == 0:
        r.bad = True
        return r
    src = t.page_src[first:first + r.k]
    j0, j1 = page_of(src, off), page_of(src, off + r.len - 1)
    if j1 < j0:
        r.bad = True
        return r
    r.j0, r.nb = j0, j1 - j0 + 1
    a = src[j0]
    if a < off:
        b = src[j0 + 1] if j0 + 1 < r.k else r.S
        r.head, r.head_bytes = True, max(min(b, off + r.len) - a, 0)
    return r


def page_ok(t, r, j):
    e = r.first + j
    a = t.page_src[e]
    b = t.page_src[e + 1] if j + 1 < r.k else r.S
    end = r.off + r.len
    if t.page_len[e] > t.page_size or a >= r.S or a >= b:
        return False
    if j == r.j0:
        if a > r.off or r.off >= b:
            return False
    elif a <= r.off or a >= end:
        return False
    return not (j == r.j0 + r.nb - 1 and b < end)


def sound(t, r):
    return not r.bad and all(page_ok(t, r, r.j0 + j) for j in range(r.nb))


class Item:
    """one touched page's work: `target` bytes of page `entry` (page_len bytes) decoded at `dst` of the range's region -- a head: into
    its scratch slot, whose bytes [copy_at, copy_at + copy_len) then go to the region's first byte"""

    def __init__(self, entry, in_len, target, head, dst, copy_at, copy_len):
        self.entry, self.in_len, self.target, self.head, self.dst, self.copy_at, self.copy_len = entry, in_len, target, head, dst, copy_at, copy_len


def items(t, r):
    """the items of a sound range, in stream order"""
    out = []
    end = r.off + r.len
    for j in range(r.j0, r.j0 + r.nb):
        e = r.first + j
        a = t.page_src[e]
        b = t.page_src[e + 1] if j + 1 < r.k else r.S
        hi = min(b, end)
        if a < r.off:
            out.append(Item(e, t.page_len[e], hi - a, True, 0, r.off - a, hi - r.off))
        else:
            out.append(Item(e, t.page_len[e], hi - a, False, a - r.off, 0, 0))
    return out


class Plan:
    """what the call decides before a page is decoded: recs, slot / head_off (the exclusive sums, one more entry for the totals), and per
    range `pre`: a final status, or None for a range whose pages are decoded"""

    def __init__(self, recs, slot, head_off, pre):
        self.recs, self.slot, self.head_off, self.pre = recs, slot, head_off, pre

    @property
    def items_needed(self):
        return self.slot[-1]

    @property
    def scratch_needed(self):
        return self.head_off[-1]


def plan(t, ranges, max_items=None, scratch_cap=None):
    """ranges = [(stream, off, len)]; None for a capacity: it suffices (MEM_HOST)"""
    recs = [locate(t, i, off, length) for i, off, length in ranges]
    slot, head_off = [0], [0]
    for r in recs:
        slot.append(slot[-1] + r.nb)
        head_off.append(head_off[-1] + r.head_slot)
    pre = []
    for q, r in enumerate(recs):
        if r.no_stream:
            pre.append(E_INVALID_ARG)
        elif r.len == 0:
            pre.append(OK)
        elif (max_items is not None and slot[q] + r.nb > max_items) or \
                (scratch_cap is not None and r.head and head_off[q] + r.head_bytes > scratch_cap):
            pre.append(E_OUTPUT_TOO_SMALL)
        elif not sound(t, r):
            pre.append(E_INVALID_ARG)
        else:
            pre.append(None)
    return Plan(recs, slot, head_off, pre)


def read(t, ranges, decode_partial, max_items=None, scratch_cap=None):
    """the whole rule: decode_partial(entry, in_len, target) -> (status, bytes) is lz4flex_decompress_batch_partial for one page.
    Returns [(status, out_len, bytes or None)]"""
    p = plan(t, ranges, max_items, scratch_cap)
    out = []
    for r, pre in zip(p.recs, p.pre):
        if pre is not None:
            out.append((pre, 0, b"" if pre == OK else None))
            continue
        buf, st = bytearray(r.len), OK
        for it in items(t, r):
            code, got = decode_partial(it.entry, it.in_len, it.target)
            if code != OK or len(got) != it.target:
                st = code if code != OK else E_EXPECTED_ANOTHER_BYTE
                break
            if it.head:
                buf[0:it.copy_len] = got[it.copy_at:it.copy_at + it.copy_len]
            else:
                buf[it.dst:it.dst + it.target] = got
        out.append((st, r.len, bytes(buf)) if st == OK else (st, 0, None))
    return out
