// paged_append_shim.cpp -- lz4_flex_amd/csrc/paged_append.h behind a C interface, for tests/test_paged_append_model.py (a CPU test: the
// header is plain integer arithmetic, compiled here without HIP).  pa_plan walks steps 1 to 4 of a call the way the device does: every
// stream located, the exclusive sums of the stage slots, who is served.  PAGED_APPEND_SHIM_MAIN: the same walk over seeded garbage tables
// as a stand-alone program (its own main) that checks what every stream that goes on may read and write, for a sanitizer build outside
// Python.
#include <cstdint>
#include <vector>

#include "../../lz4_flex_amd/csrc/paged_append.h"

using namespace lz4flex_paged;

extern "C" {

uint64_t pa_rec_bytes() { return sizeof(AppendRec); }
uint64_t pa_stage_bound(uint64_t sum_add_len, uint32_t n, uint32_t window_max) { return append_stage_bound(sum_add_len, n, window_max); }

// One call.  pre[i]: the status stream i has before a page is decoded, -1 for a stream that goes on to the reopen; out[8 i ..]: base, T,
// the stage bytes it needs, its slot (the exclusive sum), stage_off, tail_src, the first page index the rounds write, the pages it may
// take from there on.  Returns the stage bytes the call needs in all.
uint64_t pa_plan(const uint64_t* page_off, const uint32_t* page_len, const uint32_t* page_src, const uint32_t* n_pages, const uint32_t* in_done,
                 uint32_t n, uint32_t page_size, uint32_t window_max, const uint32_t* add_len, uint64_t stage_cap, int32_t* pre, uint64_t* out) {
    const AppendTables t{page_off, page_len, page_src, n_pages, in_done, n, page_size, window_max};
    uint64_t slot = 0;
    for (uint32_t i = 0; i < n; i++) {
        AppendRec r;
        append_locate(t, i, add_len[i], &r);
        const uint64_t need = append_slot_bytes(r);
        pre[i] = append_pre(r, slot, stage_cap);
        uint64_t* o = out + 8 * (uint64_t)i;
        o[0] = r.base; o[1] = r.T; o[2] = need; o[3] = slot;
        o[4] = pre[i] == -1 ? slot : NO_STAGE;
        o[5] = (r.flags & (APP_IDLE | APP_BAD)) != 0u ? r.S : r.base;
        o[6] = append_k0(r); o[7] = pre[i] == -1 ? append_room(r) : 0;
        slot += need;
    }
    return slot;
}

}  // extern "C"

#ifdef PAGED_APPEND_SHIM_MAIN
#include <cstdio>
// seeded garbage: tables of random numbers, adds of random lengths; a stream that goes on reads one entry and one page inside its own
// span, gets a stage slot inside stage_cap that holds its tail and its new bytes, and resumes at a page index inside its capacity
int main() {
    uint64_t x = 88172645463325252ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    uint64_t going = 0, refused = 0, bad = 0;
    for (int round = 0; round < 2000; round++) {
        const uint32_t n = 1 + rnd() % 6, P = 64 + rnd() % 200, window_max = P + rnd() % 3000;
        std::vector<uint64_t> page_off{rnd() % 3};
        for (uint32_t i = 0; i < n; i++) page_off.push_back(round % 7 == 6 && rnd() % 4 == 0 && page_off.back() ? page_off.back() - 1 : page_off.back() + rnd() % 9);
        uint64_t entries = 0;
        for (uint64_t v : page_off) entries = v > entries ? v : entries;
        // exactly the entries the streams own: a read outside them is a read outside the allocation
        std::vector<uint32_t> page_len(entries), page_src(entries), n_pages(n), in_done(n), add_len(n);
        const uint32_t scale = round % 2 ? 4000u : 0xFFFFFFFFu;
        for (auto& v : page_len) v = rnd() % (round % 3 ? P + 2 : scale);
        for (auto& v : page_src) v = rnd() % scale;
        for (auto& v : n_pages) v = rnd() % 10;
        for (auto& v : in_done) v = rnd() % scale;
        for (auto& v : add_len) v = rnd() % 4 == 0 ? 0u : rnd() % 5 == 0 ? (uint32_t)rnd() : (uint32_t)(rnd() % 3000);
        if (round % 4 == 0)                              // mostly sound, so that streams go on
            for (uint32_t i = 0; i < n; i++) {
                const uint64_t C = page_off[i + 1] >= page_off[i] ? page_off[i + 1] - page_off[i] : 0;
                n_pages[i] = C ? rnd() % (C + 1) : 0;
                if (n_pages[i] == 0) { in_done[i] = 0; continue; }
                const uint64_t e = page_off[i] + n_pages[i] - 1;
                page_len[e] = 1 + rnd() % P; page_src[e] = rnd() % 5000; in_done[i] = page_src[e] + 1 + rnd() % window_max;
            }
        const uint64_t stage_cap = rnd() % 3 == 0 ? ~0ull : rnd() % 9000;
        std::vector<int32_t> pre(n);
        std::vector<uint64_t> out(8 * (size_t)n);
        const uint64_t total = pa_plan(page_off.data(), page_len.data(), page_src.data(), n_pages.data(), in_done.data(), n, P, window_max,
                                       add_len.data(), stage_cap, pre.data(), out.data());
        uint64_t at = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t* o = &out[8 * (size_t)i];
            bool ok = o[3] == at && o[2] % 64 == 0;
            at += o[2];
            if (pre[i] == -1) {
                const uint64_t first = page_off[i], C = page_off[i + 1] - first, k = n_pages[i], T = o[1], A = add_len[i];
                ok = ok && page_off[i + 1] >= first && A != 0 && k <= C && o[4] == o[3] && o[2] >= T + A && o[3] + o[2] <= stage_cap && T <= window_max;
                ok = ok && o[6] == (k ? k - 1 : 0) && o[6] + o[7] == C && (uint64_t)o[0] + T + A <= 0xFFFFFFFFull && o[5] == o[0];
                if (k) {
                    const uint64_t e = first + k - 1;
                    ok = ok && e >= first && e < first + C && page_len[e] >= 1 && page_len[e] <= P && page_src[e] == o[0] && in_done[i] - o[0] == T && T >= 1;
                } else ok = ok && T == 0 && o[0] == 0 && in_done[i] == 0;
                going++;
            } else {
                ok = ok && o[4] == NO_STAGE && o[7] == 0 && (pre[i] != 0 || add_len[i] == 0) && (pre[i] != E_OUTPUT_TOO_SMALL || o[3] + o[2] > stage_cap);
                refused += pre[i] == E_OUTPUT_TOO_SMALL; bad += pre[i] == E_INVALID_ARG;
            }
            if (!ok) { std::printf("round %d: stream %u leaves its bounds\n", round, i); return 1; }
        }
        if (at != total) { std::printf("round %d: the slots do not add up\n", round); return 1; }
    }
    if (going < 300 || refused < 30 || bad < 300) { std::printf("the walk is too tame: %llu %llu %llu\n", (unsigned long long)going, (unsigned long long)refused, (unsigned long long)bad); return 1; }
    std::printf("2000 tables, %llu streams go on, %llu refused, %llu contradicting, all inside their bounds\n", (unsigned long long)going,
                (unsigned long long)refused, (unsigned long long)bad);
    return 0;
}
#endif
