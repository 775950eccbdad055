// lz4_seq_walk.h -- the tile WALK of the one-block-per-wavefront kernels: the sequence decoder (lz4_decompress_seq.hip), the size
// scan (lz4_size_scan.hip) and the fit pass (lz4_fit.hip).  All follow a block's token chain (the reference's `ip`, decompress.rs:244-332, positions only) the same
// way, and this is that way, once.
//
// The compressed stream is consumed in tiles of 3 840 bytes staged in LDS; a tile is cut into 64 parts of 60 bytes and lane k walks
// part k's chain from an ASSUMED entry, two LDS round trips per hop at most (token + first length byte; the match length byte of a
// 15-nibble), marking token positions in a 64-bit register mask.  A chain started at a wrong byte falls into step with the true chain
// after a few sequences; the exits are followed from the tile's true entry (every part leaving into the next one: a DPP move; else
// pointer jumping with ds_bpermute), parts whose entry was wrong walk again until they meet their first walk's marks (the
// parallel-chain parse of lz4_decompress_pcd.hip / lz4_decompress_plan.hip, masks only).  The set bits of the live parts, compacted
// into a u16 list in LDS, are the tile's sequences in order; decode_token reads one of them for its lane.
//
// A kernel's tile loop calls the stages in order: stage_tile, first_walks, settle_chain, write_token_list.  Everything here addresses
// LDS by byte from 0: the kernel's dynamic segment is its only LDS and begins [token list | tile | ...] (the kernel's own behind).
#pragma once
#include <stdint.h>

#include "lz4_device.h"
#include "lz4_pcd_common.h"
#include "lz4_wave_prims.h"

namespace lz4flex_dev {
namespace sw {

typedef __attribute__((address_space(3))) uint16_t lds_u16;
typedef __attribute__((address_space(3))) uint32_t lds_u32;
using pcd::X_END;
using pcd::X_ERR;

// ---- geometry -------------------------------------------------------------------------------------------------------------------
#ifndef LZ4S_PB
#define LZ4S_PB 60
#endif
constexpr uint32_t PB = LZ4S_PB;             // bytes per part (an odd number of dwords: lane k reading part k hits its own bank)
constexpr uint32_t NPART = 64u;              // parts per tile = lanes
constexpr uint32_t PT = PB * NPART;          // 3 840 compressed bytes per tile
constexpr uint32_t TPAD = 16u;               // bytes in front of the tile (the decoder's lanes read the 16 bytes that END with their literals)
constexpr uint32_t TMARGIN = 224u;           // bytes behind the tile staged with it
constexpr uint32_t TILE_LDS = TPAD + PT + TMARGIN;
constexpr uint32_t POSCAP = PT / 3u;         // sequences per tile: a sequence with a match is at least 3 bytes
constexpr uint32_t POS_LDS = (2u * POSCAP + 15u) & ~15u;
constexpr uint32_t WALK_LITMAX = 200u;       // literal run a hop steps over without the generic walker (its end stays inside the staged bytes)
constexpr uint32_t POS_LIMIT = 0xFFFF0000u;  // positions in either stream stay below this: `pos + a KiB` never wraps (a block beyond it is the second pass's)
// LDS: [token list | tile | the kernel's own]  (the tile is not first: a lane may read up to 16 bytes in front of it)
constexpr uint32_t LDS_POS = 0u, LDS_TILE = LDS_POS + POS_LDS;
static_assert(TILE_LDS % 16u == 0u && PT % 16u == 0u && POS_LDS % 16u == 0u && PB % 4u == 0u && (PB / 4u) % 2u == 1u && PB <= 64u, "geometry");
static_assert(PT - 1u + 4u + 15u + WALK_LITMAX + 4u < PT + TMARGIN, "a hop's length byte lies inside the staged bytes");

// ---- lanes and LDS --------------------------------------------------------------------------------------------------------------
// Behind a region only some lanes execute: an (empty) instruction of its own.  Without it the compiler lets the region end in the
// block where uniform paths (an early return, a loop's exit) meet as well, and then takes every value merged there -- the
// function's result, the loop's state -- for divergent: masks and counters move to vector registers, uniform branches become
// exec-mask loops (the first build of the decoder ran its whole main loop that way).
#define SW_JOIN() asm volatile("; join")
// (wave_incl_add, rdlane, uni, ctz64: lz4_wave_prims.h)
__device__ __forceinline__ uint64_t ballot(bool b) { return __builtin_amdgcn_ballot_w64(b); }
__device__ __forceinline__ bool lanes(uint64_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }      // this lane's bit of a wave-uniform mask
__device__ __forceinline__ uint64_t low_mask(uint32_t n) { return n >= 64u ? ~0ull : (1ull << n) - 1ull; }
__device__ __forceinline__ uint32_t bperm(uint32_t lane_src, uint32_t v) { return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(lane_src * 4u), (int)v); }

// LDS by byte address (the dynamic segment starts at 0)
__device__ __forceinline__ lds_u8* L8(uint32_t a) { return (lds_u8*)(uintptr_t)a; }
__device__ __forceinline__ void lds_wr16(uint32_t a, const u32x4& v) { __builtin_memcpy((void*)L8(a), &v, 16); }
__device__ __forceinline__ void lds_wr4(uint32_t a, uint32_t v) { __builtin_memcpy((void*)L8(a), &v, 4); }
__device__ __forceinline__ void lds_wr2(uint32_t a, uint32_t v) { const uint16_t t = (uint16_t)v; __builtin_memcpy((void*)L8(a), &t, 2); }
// the four bytes at LDS address a (any alignment) out of two aligned dwords
__device__ __forceinline__ uint32_t lds_rd4u(uint32_t a) {
    const lds_u32* q = (const lds_u32*)(uintptr_t)(a & ~3u);
    const uint32_t d0 = q[0], d1 = q[1];
    return __builtin_amdgcn_alignbyte(d1, d0, a & 3u);
}

// ---- the walker -----------------------------------------------------------------------------------------------------------------
// the compressed bytes for the generic sequence walker (lz4_pcd_common.h parse_seq): the staged tile from LDS, else memory
struct Reader {
    const g_u8* g;
    uint32_t t0;
    __device__ __forceinline__ uint32_t operator()(uint32_t pos) const {
        const uint32_t r = pos - t0;
        return r < PT + TMARGIN ? (uint32_t)*L8(LDS_TILE + TPAD + r) : (uint32_t)g[pos];
    }
    __device__ __forceinline__ uint32_t u32(uint32_t pos) const { return (*this)(pos) | ((*this)(pos + 1u) << 8) | ((*this)(pos + 2u) << 16) | ((*this)(pos + 3u) << 24); }
};
// where the sequence at position p ends (the next token; ilen: the block ends there), exactly, byte by byte -- the walk's rare path, kept
// out of its loop: a real call, one copy per translation unit.  X_ERR: this chain cannot be a real one.
static __device__ __noinline__ uint32_t slow_next(const g_u8* g, uint32_t t0, uint32_t ilen, uint32_t p) {
    Reader rd;
    rd.g = g; rd.t0 = t0;
    pcd::Seq q;
    const uint32_t nx = pcd::parse_seq<Reader, false>(rd, ilen, p, q);
    return nx == X_END ? ilen : nx;
}

struct Part {           // positions relative to the tile's first byte t0
    uint64_t marks;      // token positions of the standing walk, relative to the part's first byte
    uint32_t from;       // where the standing walk began (X_ERR: none)
    uint32_t exit;       // where its chain leaves the part: a position >= the part's end (>= ilen - t0: the block ends or fails there), or X_ERR
};

// One walk of a part from r (decompress.rs:244-258, 366-391: positions only).  FIRST: every position is marked.  Else: until the walk
// lands on a position the standing walk marked (its marks stand from there, and its exit) or leaves the part.  A hop is two LDS
// round trips at most: token + first length byte, and the match length byte of a 15-nibble.
template <bool FIRST>
__device__ __forceinline__ void walk_part(const g_u8* g, uint32_t t0, uint32_t ilen, uint32_t r, uint32_t p0, uint32_t pend, Part& s) {
    const uint32_t entry = r;
    const uint32_t tb = LDS_TILE + TPAD;
    uint64_t m2 = 0ull;
    uint32_t exit_ = X_ERR;
    bool merged = false;
    for (;;) {
        bool slow = false;
        uint64_t bit = 0ull;
        for (;;) {
            if (r >= pend) { exit_ = r; break; }
            bit = 1ull << (r - p0);
            if (!FIRST && (s.marks & bit) != 0ull) { merged = true; break; }
            const uint32_t w = lds_rd4u(tb + r);
            const uint32_t L = (w >> 4) & 15u, M = w & 15u, e1 = (w >> 8) & 0xFFu;
            const bool l15 = L == 15u;
            uint32_t nx = r + (l15 ? 15u + e1 + 4u : L + 3u);
            slow = l15 && e1 > WALK_LITMAX - 15u;
            if (M == 15u && !slow) {
                const uint32_t e2 = *L8(tb + nx);
                nx += 1u;
                slow = e2 == 255u;
            }
            if (slow) break;
            m2 |= bit;
            r = nx;
        }
        if (!slow) break;
        const uint32_t nx = slow_next(g, t0, ilen, t0 + r);     // (r < pend: a position of the block)
        if (nx == X_ERR) break;
        m2 |= bit;
        r = nx - t0;
    }
    if (merged) { s.marks = m2 | (s.marks & ~((1ull << (r - p0)) - 1ull)); s.from = entry; }
    else { s.marks = m2; s.from = entry; s.exit = exit_; }
}

// ---- the stages of one tile (t0: the tile's first byte, a multiple of 16; entry_r: the chain's entry relative to t0) --------------
// stage the tile: [t0, t0 + PT + TMARGIN), zeros behind the block (reads stay inside [0, ilen))
__device__ __forceinline__ void stage_tile(const g_u8* in, uint32_t ilen, uint32_t t0, uint32_t lane) {
    for (uint32_t o0 = 0u; o0 < PT + TMARGIN; o0 += 1024u) {
        const uint32_t o = o0 + 16u * lane;
        if (o < PT + TMARGIN) {
            u32x4 v = {0u, 0u, 0u, 0u};
            const uint32_t g = t0 + o;
            if (g + 16u <= ilen) __builtin_memcpy(&v, (const void*)(in + g), 16);
            else if (g < ilen) {
                uint32_t wv[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (uint32_t k = 0u; k < 16u; ++k) if (g + k < ilen) wv[k >> 2] |= (uint32_t)in[g + k] << (8u * (k & 3u));
                v = u32x4{wv[0], wv[1], wv[2], wv[3]};
            }
            lds_wr16(LDS_TILE + TPAD + o, v);
        }
        SW_JOIN();
    }
}

// first walks: lane 0 from the tile's entry, the others from their part's first byte (positions relative to t0)
__device__ __forceinline__ void first_walks(const g_u8* in, uint32_t ilen, uint32_t t0, uint32_t lane, uint32_t entry_r, Part& s) {
    const uint32_t ilr = ilen - t0;
    const uint32_t p0 = PB * lane;
    const uint32_t pend = p0 + PB < ilr ? p0 + PB : ilr;
    s.marks = 0ull; s.from = X_ERR; s.exit = X_ERR;
    if (p0 < ilr) walk_part<true>(in, t0, ilen, lane == 0u ? entry_r : p0, p0, pend, s);
    SW_JOIN();
}

// which parts does the true chain visit, and where does it enter them?  (lz4_decompress_plan.hip)  Parts whose entry was not the
// assumed one walk again, `rounds` times in all.  Returns where the chain leaves the tile (relative to t0; X_ERR: it did not
// settle); my_entry: where it enters this lane's part (X_ERR: it does not), s.marks from there on are the part's tokens.
__device__ __forceinline__ uint32_t settle_chain(const g_u8* in, uint32_t ilen, uint32_t t0, uint32_t lane, uint32_t entry_r, Part& s,
                                                 uint32_t& my_entry, uint32_t& rounds) {
    const uint32_t ilr = ilen - t0;
    const uint32_t p0 = PB * lane;
    const uint32_t pend = p0 + PB < ilr ? p0 + PB : ilr;
    my_entry = X_ERR;
    uint64_t path = 1ull;
    bool settled = false;
    const uint32_t nparts = ilr < PT ? (ilr + PB - 1u) / PB : NPART;       // parts that hold bytes of the block
    rounds = 0u;
    for (uint32_t round = 0u; round < NPART + 2u; ++round) {
        const bool inside = s.exit != X_ERR && s.exit < PT && s.exit < ilr;
        const uint32_t nxt = inside ? s.exit / PB : 64u;
        // the usual tile: every part's chain leaves into the NEXT part (no sequence is longer than a part) -- the path is all parts and
        // a part's entry is its left neighbour's exit, one DPP move; else the general form, pointer jumping over the exits
        const uint64_t chain_ok = ballot(nxt == lane + 1u || (lane + 1u >= nparts && nxt == 64u)) | ~low_mask(nparts);
        if (chain_ok == ~0ull) {
            path = low_mask(nparts);
            const uint32_t left = (uint32_t)__builtin_amdgcn_update_dpp((int)X_ERR, (int)s.exit, 0x138, 0xf, 0xf, false);   // wave_shr:1
            my_entry = lane == 0u ? entry_r : (lane < nparts ? left : X_ERR);
        } else {
            uint64_t reach = 1ull << lane;
            uint32_t jump = nxt;
#pragma unroll
            for (uint32_t i = 0u; i < 6u; ++i) {
                const uint32_t sl = jump < 64u ? jump : lane;
                const uint32_t rlo = bperm(sl, (uint32_t)reach), rhi = bperm(sl, (uint32_t)(reach >> 32)), j2 = bperm(sl, jump);
                if (jump < 64u) { reach |= ((uint64_t)rhi << 32) | rlo; jump = j2; }
            }
            path = ((uint64_t)rdlane((uint32_t)(reach >> 32), 0u) << 32) | rdlane((uint32_t)reach, 0u);
            const uint64_t before = path & ((1ull << lane) - 1ull);
            const uint32_t pred = before != 0ull ? 63u - (uint32_t)__builtin_clzll(before) : lane;
            const uint32_t pulled = bperm(pred, s.exit);
            my_entry = lane == 0u ? entry_r : (lanes(path) && before != 0ull ? pulled : X_ERR);
        }
        SW_JOIN();
        path = ((uint64_t)uni((uint32_t)(path >> 32)) << 32) | uni((uint32_t)path);
        // an entry the standing walk passed through needs no walk: its marks stand from there
        if (my_entry != X_ERR && s.from != my_entry && my_entry - p0 < 64u && ((s.marks >> (my_entry - p0)) & 1ull) != 0ull) {
            s.marks &= ~((1ull << (my_entry - p0)) - 1ull);
            s.from = my_entry;
        }
        SW_JOIN();
        const uint64_t needm = ballot(my_entry != X_ERR && s.from != my_entry);
        if (needm == 0ull) { settled = true; break; }
        if (lanes(needm)) walk_part<false>(in, t0, ilen, my_entry, p0, pend, s);
        SW_JOIN();
        rounds += 1u;
    }
    // (the compiler folds the loop's uniform exit into the divergent re-walk branch and then takes everything behind it for
    // divergent: say what is uniform)
    settled = uni(settled ? 1u : 0u) != 0u;
    path = ((uint64_t)uni((uint32_t)(path >> 32)) << 32) | uni((uint32_t)path);
    // the last part on the path says where the chain leaves the tile
    return settled ? rdlane(s.exit, 63u - (uint32_t)__builtin_clzll(path)) : X_ERR;
}

// the token list: the marks of the parts on the chain, compacted into u16 positions (relative to t0) at LDS_POS.  Returns their
// number n_tile; 0 or more than POSCAP (not a real chain): nothing is written, the kernel gives the block up
__device__ __forceinline__ uint32_t write_token_list(uint32_t lane, uint32_t my_entry, const Part& s) {
    uint64_t m = my_entry != X_ERR ? s.marks : 0ull;
    const uint32_t cnt = (uint32_t)__builtin_popcountll(m);
    const uint32_t cincl = wave_incl_add(cnt);
    const uint32_t n_tile = rdlane(cincl, 63u);
    if (n_tile > POSCAP || n_tile == 0u) return n_tile;
    uint32_t at = LDS_POS + 2u * (cincl - cnt);
    while (ballot(m != 0ull) != 0ull) {
        if (m != 0ull) {
            lds_wr2(at, PB * lane + ctz64(m));
            at += 2u;
            m &= m - 1ull;
        }
        SW_JOIN();
    }
    return n_tile;
}

// ---- a sequence of the token list, for its lane -----------------------------------------------------------------------------------
// token, lengths, offset (decompress.rs:249-258, 284, 373-391) of sequence idx, from two unaligned dword reads of the tile.  A literal
// run of more than LITMAX bytes (that covers a length byte of 255) is not a lane's: its bit in biglit, and the fields behind `lsr`
// mean nothing (the kernel asserts that PT + 1 + LITMAX + what it reads behind lies inside the staged bytes).  ilr: the block's end
// relative to t0.
struct Token {
    uint32_t tpr;               // the token's position, relative to t0
    uint32_t lit, lsr, lend;    // literal length; the literals' first byte and the byte behind them
    uint32_t off, e2, mlx, nxt; // offset, the first match length byte, match length with it, the next token
    bool l15, m15;              // a 15-nibble: the length has at least one more byte
    uint64_t biglit, lastm;     // lanes: a literal run of more than LITMAX; the block's last sequence, literals only (:366-368) -- or an error
};
template <uint32_t LITMAX>
__device__ __forceinline__ Token decode_token(uint32_t idx, uint32_t ilr) {
    const uint32_t tb = LDS_TILE + TPAD;
    Token t;
    t.tpr = (uint32_t)*(const lds_u16*)(uintptr_t)(LDS_POS + 2u * idx);
    const uint32_t w = lds_rd4u(tb + t.tpr);
    const uint32_t L = (w >> 4) & 15u, M = w & 15u, e1 = (w >> 8) & 0xFFu;
    t.l15 = L == 15u;
    t.lit = t.l15 ? 15u + e1 : L;
    t.lsr = t.tpr + (t.l15 ? 2u : 1u);
    t.biglit = ballot(t.lit > LITMAX);
    t.lend = t.lit > LITMAX ? 0u : t.lsr + t.lit;
    const uint32_t w1 = lds_rd4u(tb + t.lend);
    t.off = w1 & 0xFFFFu; t.e2 = (w1 >> 16) & 0xFFu;
    t.m15 = M == 15u;
    t.mlx = 4u + M + (t.m15 ? t.e2 : 0u);
    t.nxt = t.lend + (t.m15 ? 3u : 2u);
    t.lastm = ballot(t.lend >= ilr);
    return t;
}

// ---- a length run, by the whole wavefront (the size scan's and the fit pass's sequences that no lane takes) ------------------------------
// a length run at q (read_integer, decompress.rs:160-174 via :336-340 / :386-391), 64 bytes per load: adds its value to v, q behind it.
// false: the input ends inside the run, or v passes POS_LIMIT
__device__ __forceinline__ bool run_len(const g_u8* in, uint32_t ilen, uint32_t lane, uint32_t& q, uint32_t& v) {
    for (;;) {
        const uint32_t p = q + lane;
        const uint32_t b = p < ilen ? (uint32_t)in[p] : 255u;
        const uint64_t stop = ballot(p < ilen && b != 255u);
        SW_JOIN();
        if (stop != 0ull) {
            const uint32_t k = ctz64(stop);
            const uint64_t add = 255ull * k + rdlane(b, k);
            if ((uint64_t)v + add > POS_LIMIT) return false;
            v += (uint32_t)add;
            q += k + 1u;
            return true;
        }
        if (ilen - q <= 64u) return false;
        if ((uint64_t)v + 255u * 64u > POS_LIMIT) return false;
        v += 255u * 64u;
        q += 64u;
    }
}

// One sequence of any shape at ip by the whole wavefront, in the reference's check order (decompress.rs:334-443), lengths only.  op: bytes
// produced in front of it (advanced); hist: bytes in front of the block's output an offset may reach; lit, ml: its lengths.  false: an
// error, or a position beyond POS_LIMIT -- the kernel's serial pass names it.  last: the block ended here (ml = 0).
static __device__ bool wave_seq(const g_u8* in, uint32_t ilen, uint32_t lane, uint32_t hist, uint32_t ip, uint32_t& op, uint32_t& lit,
                                uint32_t& ml, bool& last) {
    const uint32_t t = uni(in[ip]);
    ip += 1u;
    lit = t >> 4;
    ml = 0u;
    if (lit == 15u && !run_len(in, ilen, lane, ip, lit)) return false;
    if (lit > ilen - ip || (uint64_t)op + lit > POS_LIMIT) return false;
    op += lit;
    ip += lit;
    if (ip >= ilen) { last = true; return true; }
    if (ilen - ip < 2u) return false;
    const uint32_t offset = uni((uint32_t)in[ip] | ((uint32_t)in[ip + 1u] << 8));
    ip += 2u;
    if (offset == 0u) return false;
    ml = 4u + (t & 15u);
    if (ml == 19u && !run_len(in, ilen, lane, ip, ml)) return false;
    if ((uint64_t)offset > (uint64_t)op + hist) return false;
    if ((uint64_t)op + ml > POS_LIMIT) return false;
    op += ml;
    if (ip >= ilen) return false;              // a match is always followed by another token (:439-443)
    return true;
}

// ---- what a chunk of 64 decoded tokens says, one ballot per reference check (ilr: the block's end relative to t0) -------------------------
// errm: lanes whose sequence fails a check that needs no position (literals past the input :336-340 / :346-348, an offset missing
// :373-375, no token behind a match :439-443, offset zero :168-173); bigm: lanes whose sequence has more length bytes than a lane reads
__device__ __forceinline__ void chunk_masks(const Token& t, uint32_t ilr, uint64_t& errm, uint64_t& bigm) {
    errm = ballot(t.l15 && t.tpr + 1u >= ilr) | ballot(t.lend > ilr) |
           (~t.lastm & (ballot(t.lend + 2u > ilr) | ballot(t.nxt >= ilr) | ballot(t.off == 0u)));
    bigm = t.biglit | (~t.lastm & ballot(t.m15 && t.e2 == 255u));
}

// ---- the serial passes' length run: read_integer (decompress.rs:160-174), 64-bit positions ------------------------------------------------
__device__ __forceinline__ int32_t read_integer(const uint8_t* in, uint64_t ilen, uint64_t& ip, uint64_t& v) {   // :160-174
    for (;;) {
        if (ip >= ilen) return LZ4FLEX_DEV_E_EXPECTED_ANOTHER_BYTE;
        const uint32_t extra = in[ip++];
        v += extra;
        if (extra != 0xFFu) return 0;
    }
}

}  // namespace sw
}  // namespace lz4flex_dev
