// paged_range_shim.cpp -- lz4_flex_amd/csrc/paged_range.h behind a C interface, for tests/test_paged_read_model.py (a CPU test: the
// header is plain integer arithmetic, compiled here without HIP).  pr_plan walks a call the way the device does: every range located, the
// two exclusive sums, who is served, whether the touched pages agree with the rule, then every item.  PAGED_RANGE_SHIM_MAIN: the same
// walk over seeded garbage tables as a stand-alone program (its own main) that checks every item's bounds, for a sanitizer build
// outside Python.
#include <cstdint>
#include <vector>

#include "../../lz4_flex_amd/csrc/paged_range.h"

using namespace lz4flex_paged;

extern "C" {

uint64_t pr_rec_bytes() { return sizeof(RangeRec); }
uint32_t pr_pages_bound(uint32_t len, uint32_t page_size) { return pages_bound(len, page_size); }
uint32_t pr_lfit_page(uint32_t page_size) { return lfit_page(page_size); }

// out[0 .. 8): clipped length, j0, nb, head, head_bytes, bad (locate's own finding), no_stream, k
void pr_locate(const uint64_t* page_off, const uint32_t* page_len, const uint32_t* page_src, const uint32_t* n_pages, const uint32_t* in_done,
               uint32_t n, uint32_t page_size, uint32_t i, uint32_t off, uint32_t len, uint64_t* out) {
    const Tables t{page_off, page_len, page_src, n_pages, in_done, n, page_size};
    RangeRec r;
    locate(t, i, off, len, &r);
    out[0] = r.len; out[1] = r.j0; out[2] = r.nb; out[3] = (r.flags & REC_HEAD) ? 1 : 0; out[4] = r.head_bytes;
    out[5] = (r.flags & REC_BAD) ? 1 : 0; out[6] = (r.flags & REC_NO_STREAM) ? 1 : 0; out[7] = r.k;
}

// One call.  pre[r]: the status a range has before a page is decoded, -1 for a range whose pages are decoded; sums[2 r ..]: slot,
// head_off; items[8 q ..] for item q, ranges in order, pages in stream order: range, in_off, in_len, target, head, out_off (a body:
// relative to the range's region; a head: in the scratch), copy_at, copy_len.  Returns the number of items (at most item_cap are written).
uint64_t pr_plan(const uint64_t* page_off, const uint32_t* page_len, const uint32_t* page_src, const uint32_t* n_pages, const uint32_t* in_done,
                 uint32_t n, uint32_t page_size, const uint32_t* sid, const uint32_t* off, const uint32_t* len, uint32_t m, uint64_t max_items,
                 uint64_t scratch_cap, int32_t* pre, uint64_t* sums, uint64_t* items, uint64_t item_cap) {
    const Tables t{page_off, page_len, page_src, n_pages, in_done, n, page_size};
    std::vector<RangeRec> recs(m);
    uint64_t slot = 0, head_off = 0, q = 0;
    for (uint32_t r = 0; r < m; r++) {
        RangeRec& x = recs[r];
        locate(t, sid[r], off[r], len[r], &x);
        sums[2 * r] = slot; sums[2 * r + 1] = head_off;
        const uint64_t my_slot = slot, my_head = head_off;
        slot += x.nb; head_off += head_slot_bytes(x);
        if (x.flags & REC_NO_STREAM) { pre[r] = E_INVALID_ARG; continue; }
        if (x.len == 0) { pre[r] = 0; continue; }
        if (!served(x, my_slot, my_head, max_items, scratch_cap)) { pre[r] = E_OUTPUT_TOO_SMALL; continue; }
        bool ok = (x.flags & REC_BAD) == 0;
        for (uint32_t j = 0; ok && j < x.nb; j++) ok = page_ok(t, x, x.j0 + j);
        if (!ok) { pre[r] = E_INVALID_ARG; continue; }
        pre[r] = -1;
        for (uint32_t j = 0; j < x.nb; j++) {
            Item it;
            if (!item_of(t, x, x.j0 + j, 0, my_head, &it)) { pre[r] = -2; break; }       // (never: page_ok said yes)
            if (q < item_cap) {
                uint64_t* o = items + 8 * q;
                o[0] = r; o[1] = it.in_off; o[2] = it.in_len; o[3] = it.target; o[4] = it.head ? 1 : 0; o[5] = it.out_off; o[6] = it.copy_at;
                o[7] = it.copy_len;
            }
            q++;
        }
    }
    sums[2 * (uint64_t)m] = slot; sums[2 * (uint64_t)m + 1] = head_off;
    return q;
}

}  // extern "C"

#ifdef PAGED_RANGE_SHIM_MAIN
#include <cstdio>
#include <cstdlib>
// seeded garbage: tables of random numbers, ranges of random numbers; no item may leave its stream's entries, its range's region or its head slot
int main() {
    uint64_t x = 88172645463325252ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    uint64_t total_items = 0, planned = 0;
    for (int round = 0; round < 1000; round++) {
        const uint32_t n = 1 + rnd() % 5, P = 64 + rnd() % 200;
        std::vector<uint64_t> page_off{rnd() % 3};
        for (uint32_t i = 0; i < n; i++) page_off.push_back(page_off.back() + rnd() % 9);
        const uint64_t entries = page_off.back();
        std::vector<uint32_t> page_len(entries + 1), page_src(entries + 1), n_pages(n), in_done(n);
        const uint32_t scale = round % 2 ? 1000u : 0xFFFFFFFFu;
        for (auto& v : page_len) v = rnd() % (round % 3 ? P + 2 : scale);
        for (auto& v : page_src) v = rnd() % scale;
        if (round % 4 == 0)                            // mostly ascending, so that ranges get planned
            for (uint32_t i = 0; i < n; i++) { uint32_t at = 0; for (uint64_t e = page_off[i]; e < page_off[i + 1]; e++) { page_src[e] = at; at += 1 + rnd() % 300; } }
        for (auto& v : n_pages) v = rnd() % 12;
        for (auto& v : in_done) v = rnd() % (round % 4 == 0 ? 2000u : scale);
        const uint32_t m = 40;
        std::vector<uint32_t> sid(m), off(m), len(m);
        for (uint32_t r = 0; r < m; r++) { sid[r] = rnd() % (n + 1); off[r] = rnd() % (round % 4 == 0 ? 2100u : scale); len[r] = rnd() % 5 == 0 ? 0xFFFFFFFFu : rnd() % 900; }
        std::vector<int32_t> pre(m);
        std::vector<uint64_t> sums(2 * (m + 1)), items(8 * 4096);
        const uint64_t max_items = rnd() % 60, scratch_cap = rnd() % 4000;
        const uint64_t q = pr_plan(page_off.data(), page_len.data(), page_src.data(), n_pages.data(), in_done.data(), n, P, sid.data(), off.data(),
                                   len.data(), m, max_items, scratch_cap, pre.data(), sums.data(), items.data(), 4096);
        if (q > 4096 || q > max_items) { std::printf("round %d: %llu items\n", round, (unsigned long long)q); return 1; }
        for (uint64_t k = 0; k < q; k++) {
            const uint64_t* o = &items[8 * k];
            const uint32_t r = (uint32_t)o[0], i = sid[r];
            uint64_t out[8];
            pr_locate(page_off.data(), page_len.data(), page_src.data(), n_pages.data(), in_done.data(), n, P, i, off[r], len[r], out);
            const uint64_t e = o[1] / P;
            bool ok = pre[r] == -1 && o[1] % P == 0 && e >= page_off[i] && e < page_off[i + 1] && o[2] <= P && o[3] >= 1;
            if (o[4]) ok = ok && o[5] == sums[2 * r + 1] && o[3] <= out[4] && o[5] + o[3] <= scratch_cap && o[6] + o[7] <= o[3] && o[7] <= out[0];
            else ok = ok && o[5] + o[3] <= out[0];
            if (!ok) { std::printf("round %d: item %llu of range %u leaves its bounds\n", round, (unsigned long long)k, r); return 1; }
        }
        total_items += q;
        for (uint32_t r = 0; r < m; r++) planned += pre[r] == -1;
    }
    std::printf("1000 tables, %llu ranges planned, %llu items, all inside their bounds\n", (unsigned long long)planned, (unsigned long long)total_items);
    return 0;
}
#endif
