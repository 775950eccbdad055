// paged_append.h -- the integer rule of an append to paged streams (lz4flex_paged_append, include/lz4flex_amd.h): whether stream i takes
// part, whether its table contradicts itself, where its reopened tail page lies and how many bytes it decodes to, how much of the
// caller's stage buffer it needs and whether the call's stage_cap serves it, what the tail decode said, and where the rounds resume.
// Plain functions over the tables, compiled for the host (capi.cpp: the MEM_HOST path; tests/sim/paged_append_shim.cpp: a CPU alone, no
// HIP header) and for the device (lz4_paged_append.hip: the same functions in the kernels), so there is ONE copy of the rule in C++;
// tests/paged_append_model.py is the same rule as a program.
//
// The tables may hold anything (MEM_DEVICE: caller-supplied device memory).  What is guaranteed whatever they hold: locate() reads
// page_len / page_src at one entry, `first + k - 1` with `1 <= k <= C`, so inside the stream's [first, first + C); the tail item reads
// inside that page's [e * P, e * P + P) and writes inside [0, T) of the stream's stage slot of roundup64(T + A) bytes; the rounds start at
// page index k - 1 < C.  Every check of locate() is made before an item exists.
#pragma once
#include <stdint.h>

#include "paged_range.h"

namespace lz4flex_paged {

constexpr uint32_t STAGE_ALIGN = 64u;               // a stream's stage slot starts at a multiple of this and is a multiple of it long
constexpr uint64_t NO_STAGE = ~0ull;                // stage_off[i] of a stream without a slot
enum : uint32_t {
    APP_IDLE = 1u,        // add_len[i] == 0: the stream takes no part
    APP_BAD = 2u,         // the table contradicts itself for this stream (E_INVALID_ARG, nothing written)
    APP_SERVED = 4u,      // the stream has its stage slot (set once the sum is known)
};

// the tables of an append (every array in one memory kind); n_pages and in_done are read here and written by the rounds
struct AppendTables {
    const uint64_t* page_off;     // n + 1, entries
    const uint32_t* page_len;     // per entry
    const uint32_t* page_src;     // per entry
    const uint32_t* n_pages;      // per stream
    const uint32_t* in_done;      // per stream
    uint32_t n, page_size, window_max;
};

// One stream, located (40 bytes on both sides).
struct AppendRec {
    uint64_t first;       // page_off[i]
    uint64_t C;           // page_off[i+1] - first (0 where page_off counts down)
    uint32_t k, S;        // n_pages[i], in_done[i] on entry
    uint32_t A;           // add_len[i]
    uint32_t base;        // page_src of the reopened entry (0 with k == 0): the stream position of the tail's first byte
    uint32_t T;           // S - base: the bytes the tail page decodes to (0 with k == 0)
    uint32_t flags;
};
static_assert(sizeof(AppendRec) == 40, "AppendRec is 40 bytes on both sides");

// Stream i with A new bytes: steps 1 to 3 of the rule.  With APP_IDLE or APP_BAD base and T are 0.
LZ4FLEX_PAGED_FN void append_locate(const AppendTables& t, uint32_t i, uint32_t A, AppendRec* r) {
    const uint64_t first = t.page_off[i], next = t.page_off[i + 1u];
    const uint32_t k = t.n_pages[i], S = t.in_done[i];
    r->first = first; r->C = next >= first ? next - first : 0ull; r->k = k; r->S = S; r->A = A; r->base = 0u; r->T = 0u; r->flags = 0u;
    if (A == 0u) { r->flags = APP_IDLE; return; }
    r->flags = APP_BAD;
    if (next < first || (uint64_t)k > r->C) return;
    if ((uint64_t)S + A > 0xFFFFFFFFull) return;
    if (k == 0u) {
        if (S != 0u) return;
        r->flags = 0u;
        return;
    }
    const uint64_t e = first + (k - 1u);
    const uint32_t len = t.page_len[e], src = t.page_src[e];
    if (len == 0u || len > t.page_size || src >= S || S - src > t.window_max) return;
    r->base = src; r->T = S - src; r->flags = 0u;
}

// the stage bytes the stream needs: roundup64(T + A); 0 for a stream that takes no part or was refused
LZ4FLEX_PAGED_FN uint64_t append_slot_bytes(const AppendRec& r) {
    if ((r.flags & (APP_IDLE | APP_BAD)) != 0u) return 0ull;
    return ((uint64_t)r.T + r.A + (STAGE_ALIGN - 1u)) / STAGE_ALIGN * STAGE_ALIGN;
}

// slot: the exclusive sum of append_slot_bytes over the streams in front
LZ4FLEX_PAGED_FN bool append_served(const AppendRec& r, uint64_t slot, uint64_t stage_cap) {
    const uint64_t need = append_slot_bytes(r);
    return slot <= stage_cap && need <= stage_cap - slot;
}

// the status a stream has before its tail page is decoded; -1: it goes on (steps 1, 2 and 4)
LZ4FLEX_PAGED_FN int32_t append_pre(const AppendRec& r, uint64_t slot, uint64_t stage_cap) {
    if ((r.flags & APP_IDLE) != 0u) return 0;
    if ((r.flags & APP_BAD) != 0u) return E_INVALID_ARG;
    return append_served(r, slot, stage_cap) ? -1 : E_OUTPUT_TOO_SMALL;
}

// the first page index the rounds write, and the pages the stream may take from there on
LZ4FLEX_PAGED_FN uint32_t append_k0(const AppendRec& r) { return r.k != 0u ? r.k - 1u : 0u; }
LZ4FLEX_PAGED_FN uint64_t append_room(const AppendRec& r) { return r.C - append_k0(r); }

// the bound of the stage buffer: every stream's tail is at most a window, every slot is rounded up to 64
LZ4FLEX_PAGED_FN uint64_t append_stage_bound(uint64_t sum_add_len, uint32_t n, uint32_t window_max) {
    return sum_add_len + (uint64_t)n * ((uint64_t)window_max + (STAGE_ALIGN - 1u));
}

}  // namespace lz4flex_paged
