// frame_range.h -- what a range read of an indexed frame (frame_index.cpp: lz4flex_frame_read_ranges) decides on the host: where content
// bytes [off, off + len) of a frame lie in its block table, and how many ranges one pass takes.  Pure integer functions over the
// index's HOST tables (content_off: blocks + 1 exclusive sums of the decoded sizes; len_word: the BlockInfo words): host only, no HIP;
// the record they fill is the only thing that travels to the device per range (frame_range.hip reads it).
// tests/test_frame_range_plan.py walks them on a CPU against Python's bisect, past 4 GiB of content.
#pragma once
#include <cstddef>
#include <cstdint>

namespace lz4flex_range {

constexpr uint32_t STORED_BIT = 0x80000000u;        // BlockInfo: the payload is the block itself
constexpr uint64_t HEAD_ALIGN = 64;                 // a head's scratch slot starts at a multiple of this
constexpr uint64_t PASS_SLOTS_MAX = 1ull << 24;     // touched blocks per pass (the item arrays are sized from it)

// One range of one pass, as the device sees it (64 bytes).
struct RangeRec {
    uint64_t off;         // first wanted content byte (untouched by clipping)
    uint64_t len;         // clipped length: min(range_len, S - off), 0 behind the end
    uint64_t out_off;     // where the bytes go, relative to the pass's output base
    int64_t shift;        // payload position in the pass's input base minus payload_off (0: the base is the frame itself)
    uint64_t head_off;    // a head's slot in the pass's scratch
    uint32_t b0;          // first touched block
    uint32_t nb;          // touched blocks (0 with len 0)
    uint32_t slot;        // its first item slot in the pass
    uint32_t head;        // 1: block b0 is compressed and wanted from a byte s > 0 on: it is decoded into scratch up to its last wanted byte
    uint64_t head_bytes;  // that last wanted byte's offset in the block + 1 (the head's decode target); 0 without a head
};
static_assert(sizeof(RangeRec) == 64, "RangeRec is 64 bytes on both sides");

// the clipped length of a read at end of file
inline uint64_t clip_len(uint64_t off, uint64_t len, uint64_t S) {
    if (off >= S) return 0;
    return len < S - off ? len : S - off;
}

// the block that holds content byte `pos` (pos < content_off[n]): the LAST b with content_off[b] <= pos -- blocks that decode to
// nothing share their offset with the block behind them and are stepped over
inline uint32_t block_of(const uint64_t* content_off, uint32_t n, uint64_t pos) {
    uint32_t lo = 0, hi = n;                          // invariant: content_off[lo] <= pos < content_off[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (content_off[mid] <= pos) lo = mid; else hi = mid;
    }
    return lo;
}

// Range (off, len) of a frame of n blocks: fills off / len / b0 / nb / head / head_bytes of *r (slot, head_off, out_off, shift are the
// pass's business).
inline void locate(const uint64_t* content_off, const uint32_t* len_word, uint32_t n, uint64_t off, uint64_t len, RangeRec* r) {
    const uint64_t S = content_off[n];
    r->off = off;
    r->len = clip_len(off, len, S);
    r->b0 = 0; r->nb = 0; r->head = 0; r->head_bytes = 0;
    if (r->len == 0) return;
    const uint32_t b0 = block_of(content_off, n, off), b1 = block_of(content_off, n, off + r->len - 1);
    r->b0 = b0; r->nb = b1 - b0 + 1;
    const uint64_t s = off - content_off[b0];
    if (s > 0 && !(len_word[b0] & STORED_BIT)) {
        const uint64_t end = off + r->len, bend = content_off[b0 + 1];
        r->head = 1;
        r->head_bytes = (end < bend ? end : bend) - content_off[b0];
    }
}

inline uint64_t head_slot_bytes(const RangeRec& r) { return (r.head_bytes + HEAD_ALIGN - 1) / HEAD_ALIGN * HEAD_ALIGN; }

// Passes: ranges [first, first + count) whose costs (cost[i] bytes of scratch each, the caller's sum of what range i stages) add up
// to at most pass_bytes and whose touched blocks to at most PASS_SLOTS_MAX -- but at least one range.  Fills slot and head_off of the
// pass's records and returns count; *slots / *head_total receive the pass's item slots and head scratch.
inline uint32_t cut_pass(RangeRec* recs, const uint64_t* cost, uint32_t first, uint32_t m, uint64_t pass_bytes, uint64_t* slots, uint64_t* head_total) {
    uint64_t bytes = 0, sl = 0, heads = 0;
    uint32_t i = first;
    for (; i < m; i++) {
        RangeRec& r = recs[i];
        if (i > first && (bytes > pass_bytes || cost[i] > pass_bytes - bytes || sl + r.nb > PASS_SLOTS_MAX)) break;
        r.slot = (uint32_t)sl;
        r.head_off = heads;
        sl += r.nb; heads += head_slot_bytes(r);
        bytes = cost[i] > ~0ull - bytes ? ~0ull : bytes + cost[i];
    }
    *slots = sl; *head_total = heads;
    return i - first;
}

}  // namespace lz4flex_range
