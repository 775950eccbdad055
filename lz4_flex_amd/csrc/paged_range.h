// paged_range.h -- the integer rule of a range read of paged streams (lz4flex_paged_read_ranges, include/lz4flex_amd.h): where bytes
// [off, off + len) of stream i lie in the page table lz4flex_compress_paged wrote, which page is a head, what one touched page's decode
// item is, whether the table contradicts itself for a range, who is served by the call's capacities, and the pages bound.  Plain
// functions over the tables, compiled for the host (capi.cpp: the MEM_HOST path; tests/sim/paged_range_shim.cpp: a CPU alone, no HIP
// header) and for the device (lz4_paged_read.hip: the same functions in the kernels), so there is ONE copy of the rule in C++;
// tests/paged_read_model.py is the same rule as a program.
//
// The tables may hold anything (MEM_DEVICE: caller-supplied device memory).  What is guaranteed whatever they hold: locate() touches
// table entries inside the stream's [first, first + C) only; an item that item_of() returns reads inside page e's [e * P, e * P + P) with
// e in that span and writes inside its range's [0, len) or its head slot's [0, head_bytes).  page_ok() is the condition that makes it so.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LZ4FLEX_PAGED_FN __host__ __device__ inline
#else
#define LZ4FLEX_PAGED_FN inline
#endif

namespace lz4flex_paged {

constexpr uint32_t HEAD_ALIGN = 64u;                // a head's scratch slot starts at a multiple of this
constexpr uint32_t PAGE_MIN = 64u, PAGE_MAX = 4u << 20;
constexpr int32_t E_OUTPUT_TOO_SMALL = 1, E_EXPECTED_ANOTHER_BYTE = 3, E_INVALID_ARG = 64;     // the header's LZ4FLEX_E_*
enum : uint32_t {
    REC_HEAD = 1u,        // page j0 is wanted from a byte s > 0 on: it is decoded into scratch up to its last wanted byte
    REC_BAD = 2u,         // the table contradicts itself for this range (E_INVALID_ARG, nothing written)
    REC_NO_STREAM = 4u,   // range_stream[r] >= n
    REC_SERVED = 8u,      // the range has its item slots and its head slot (set once both sums are known)
};

// what lz4flex_compress_paged produced (every array in one memory kind)
struct Tables {
    const uint64_t* page_off;     // n + 1, entries
    const uint32_t* page_len;     // per entry
    const uint32_t* page_src;     // per entry
    const uint32_t* n_pages;      // per stream
    const uint32_t* in_done;      // per stream
    uint32_t n, page_size;
};

// One range, located (48 bytes on both sides).
struct RangeRec {
    uint64_t first;       // page_off[stream]
    uint32_t stream;
    uint32_t off;         // first wanted byte (untouched by clipping)
    uint32_t len;         // clipped length: min(range_len, S - off), 0 at or behind S
    uint32_t k;           // min(n_pages, C)
    uint32_t S;           // in_done
    uint32_t j0, nb;      // touched pages j0 .. j0 + nb - 1 of the stream (nb 0 with len 0)
    uint32_t head_bytes;  // REC_HEAD: min(range end, page end) - page start, the head's decode target; else 0
    uint32_t flags;
    uint32_t pad;
};
static_assert(sizeof(RangeRec) == 48, "RangeRec is 48 bytes on both sides");

// One touched page's work: `target` bytes of the block pages[in_off .. + in_len) decoded to out_off -- relative to the output for a
// body, to the scratch for a head, whose bytes [copy_at, copy_at + copy_len) then go to the range's first byte.
struct Item {
    uint64_t in_off, out_off;
    uint32_t in_len, target;
    uint32_t copy_at, copy_len;
    bool head;
};

// Lfit(r, infinity) of the fit rule: the largest L with tail(L) <= r (r >= 1) -- what a page of literals alone holds
LZ4FLEX_PAGED_FN uint32_t lfit_page(uint32_t r) {
    if (r <= 16u) return (r - 1u) < 14u ? r - 1u : 14u;
    const uint32_t y = r - 17u;
    return 15u + y - (y >> 8) - ((y & 255u) == 255u ? 1u : 0u);
}

// the pages a range of L bytes can touch in a table lz4flex_compress_paged wrote: its first and its last page hold at least one of its
// bytes each, every page between them is a non-final page of its stream and holds at least lfit_page(P) bytes.  0: a page size the
// paged entry refuses.
LZ4FLEX_PAGED_FN uint32_t pages_bound(uint32_t L, uint32_t P) {
    if (P < PAGE_MIN || P > PAGE_MAX) return 0u;
    if (L < 2u) return L;
    return 2u + (L - 2u) / lfit_page(P);
}

LZ4FLEX_PAGED_FN uint32_t clip_len(uint32_t off, uint32_t len, uint32_t S) {
    if (off >= S) return 0u;
    return len < S - off ? len : S - off;
}

// the page that holds stream byte `pos`: the LAST j < k with src[j] <= pos (k >= 1; 0 when there is none).  src: the stream's slice
// of page_src.  A table that does not ascend gives some j < k.
LZ4FLEX_PAGED_FN uint32_t page_of(const uint32_t* src, uint32_t k, uint32_t pos) {
    uint32_t lo = 0u, hi = k;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (src[mid] <= pos) lo = mid; else hi = mid;
    }
    return lo;
}

// Range (i, off, len): every member of *r but REC_SERVED (the call's sums) and what page_ok() finds (REC_BAD is set here only for a
// range that has bytes and no pages, or whose last page lies in front of its first).
LZ4FLEX_PAGED_FN void locate(const Tables& t, uint32_t i, uint32_t off, uint32_t len, RangeRec* r) {
    r->first = 0ull; r->stream = i; r->off = off; r->len = 0u; r->k = 0u; r->S = 0u; r->j0 = 0u; r->nb = 0u; r->head_bytes = 0u;
    r->flags = 0u; r->pad = 0u;
    if (i >= t.n) { r->flags = REC_NO_STREAM; return; }
    const uint64_t first = t.page_off[i], next = t.page_off[i + 1u];
    const uint64_t C = next > first ? next - first : 0ull;
    const uint32_t np = t.n_pages[i];
    const uint32_t k = (uint64_t)np < C ? np : (uint32_t)C;
    const uint32_t S = t.in_done[i];
    r->first = first; r->k = k; r->S = S;
    r->len = clip_len(off, len, S);
    if (r->len == 0u) return;
    if (k == 0u) { r->flags = REC_BAD; return; }
    const uint32_t* src = t.page_src + first;
    const uint32_t last = off + (r->len - 1u);
    const uint32_t j0 = page_of(src, k, off), j1 = page_of(src, k, last);
    if (j1 < j0) { r->flags = REC_BAD; return; }
    r->j0 = j0; r->nb = j1 - j0 + 1u;
    const uint32_t a = src[j0];
    if (a < off) {
        const uint64_t end = (uint64_t)off + r->len;
        const uint64_t b = j0 + 1u < k ? src[j0 + 1u] : S;
        const uint64_t hi = b < end ? b : end;
        r->flags = REC_HEAD;
        r->head_bytes = hi > a ? (uint32_t)(hi - a) : 0u;
    }
}

LZ4FLEX_PAGED_FN uint64_t head_slot_bytes(const RangeRec& r) {
    return ((uint64_t)r.head_bytes + (HEAD_ALIGN - 1u)) / HEAD_ALIGN * HEAD_ALIGN;
}

// The capacities.  slot / head_off: the exclusive sums of nb / head_slot_bytes over the ranges in front.  A range without a head takes
// no scratch and is never refused for it.
LZ4FLEX_PAGED_FN bool served(const RangeRec& r, uint64_t slot, uint64_t head_off, uint64_t max_items, uint64_t scratch_cap) {
    if (slot + r.nb > max_items) return false;
    return (r.flags & REC_HEAD) == 0u || head_off + r.head_bytes <= scratch_cap;
}

// Page j (j0 <= j < j0 + nb) of a located range agrees with the rule: it holds at most a page of bytes, starts in front of S and in
// front of the page behind it, the first page holds the range's first byte, every other page starts inside the range, the last page
// reaches the range's end.
LZ4FLEX_PAGED_FN bool page_ok(const Tables& t, const RangeRec& r, uint32_t j) {
    const uint64_t e = r.first + j;
    const uint64_t a = t.page_src[e], b = j + 1u < r.k ? t.page_src[e + 1u] : r.S;
    const uint64_t end = (uint64_t)r.off + r.len;
    if (t.page_len[e] > t.page_size) return false;
    if (a >= r.S || a >= b) return false;
    if (j == r.j0) { if (a > r.off || r.off >= b) return false; }
    else if (a <= r.off || a >= end) return false;
    if (j == r.j0 + r.nb - 1u && b < end) return false;
    return true;
}

// the item of page j; false (and nothing filled) where page_ok() says no.  out_off: the range's place in the output; head_off: its
// head slot's place in the scratch
LZ4FLEX_PAGED_FN bool item_of(const Tables& t, const RangeRec& r, uint32_t j, uint64_t out_off, uint64_t head_off, Item* it) {
    if (j < r.j0 || j - r.j0 >= r.nb || !page_ok(t, r, j)) return false;
    const uint64_t e = r.first + j;
    const uint64_t a = t.page_src[e], b = j + 1u < r.k ? t.page_src[e + 1u] : r.S;
    const uint64_t end = (uint64_t)r.off + r.len;
    const uint64_t hi = b < end ? b : end;
    it->in_off = e * (uint64_t)t.page_size;
    it->in_len = t.page_len[e];
    it->target = (uint32_t)(hi - a);
    it->head = a < r.off;
    if (it->head) {
        if ((r.flags & REC_HEAD) == 0u || it->target > r.head_bytes) return false;      // (the slot was sized from another table state)
        it->out_off = head_off; it->copy_at = (uint32_t)(r.off - a); it->copy_len = (uint32_t)(hi - r.off);
    } else {
        it->out_off = out_off + (a - r.off); it->copy_at = 0u; it->copy_len = 0u;
    }
    return true;
}

// the verdict of one item that was decoded: 0 or the range's status by rule 5
LZ4FLEX_PAGED_FN int32_t item_verdict(int32_t st, uint32_t got, uint32_t target) {
    if (st != 0) return st;
    return got != target ? E_EXPECTED_ANOTHER_BYTE : 0;
}

}  // namespace lz4flex_paged
