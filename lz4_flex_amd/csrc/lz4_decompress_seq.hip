// lz4_decompress_seq.hip -- batched LZ4 block decoder, one block per wavefront, ONE LANE PER SEQUENCE ("sequence decoder"), gfx950.
//
// What it replaces: lz4_flex::block::decompress_into / decompress_internal (src/block/decompress.rs:201-449) for many independent
// blocks.  Output bytes are the reference's; an irregular block (every error of src/block/mod.rs:82-98, a sink too small, an offset
// behind the output) is NOT diagnosed here: it is marked and the reference-order decoder of lz4_decompress.hip decodes it again and
// reports the exact error variant and detail (the scheme of lz4_decompress_pcd.hip).
//
// Round 6.  Every other batch decoder in this tree walks a block's token chain with ONE lane and copies its pieces with one
// group of four lanes: the kernel's time is one block's chain (3 380 sequences x ~630 dependent wave-instructions).
// Here nothing is done a sequence at a time:
//   * WALK (lz4_seq_walk.h, shared with the size scan lz4_size_scan.hip): the compressed stream is consumed in tiles of 3 840 bytes
//     staged in LDS, 64 lanes walk the 64 parts of a tile from assumed entries, the true chain is settled from the tile's entry, and
//     the set bits of the live parts, compacted into a u16 list in LDS, are the tile's sequences in order.  The tile loop below calls
//     its stages (stage_tile, first_walks, settle_chain, write_token_list); setup_chunk reads a sequence with decode_token.
//   * CHUNKS of 64 consecutive sequences, lane = sequence: token, lengths and offset from two aligned dword-pair reads of the
//     tile (decompress.rs:249-258, 284, 373-391), a DPP prefix sum of literal + match lengths places all 64 in the output at
//     once, every reference check that needs the position (offset <= position :286-289 / :398-402, capacity :346-356) is one
//     ballot.  Literals (<= 64 bytes) are copied by their lane, 16 bytes per access, exact length.  Matches: a source older than
//     the LDS window comes from the written-back output (loads issued at set-up, a chunk ahead of their use); a source in
//     the window copies in ROUNDS -- a lane is ready when every sequence that starts before its source's end is done (the done
//     PREFIX: one v_readlane + one compare per round), all ready lanes copy at once.  A round costs its instructions whatever
//     the number of ready lanes; JSON tiles need ~12 rounds per chunk, text ~5 (tools/chunk_study.py).
//   * the output lives in a linear LDS WINDOW (3.5 KiB) that slides by copying its last 1 280 bytes down; what leaves it has been
//     written back 16 bytes per lane.  Sequences that do not fit a lane (literal runs > 64, matches > 273 bytes or overlapping
//     their source, far matches > 64, anything with more than one length byte) are executed ALONE by the whole wavefront
//     (exact_seq: decompress.rs:334-443 for one sequence of any shape) and cut the chunk in front of them.
// PARTIAL form (lz4flex_decompress_batch_partial: the first target[b] bytes of block b; PARTIAL with NoDict, no prefix): the
// block's "capacity" is its TARGET and reaching it is the normal end.  setup_chunk cuts a chunk in front of the first sequence that
// reaches or crosses the target -- before any of the chunk's checks are looked at, so nothing behind the stop can be an error -- and that
// sequence is executed alone by the wavefront (exact_seq_partial: the reference's checks in their order, the copy clipped to the target,
// status 0, no "a match is followed by a token" check for a match that ends at the target).  run_chunks and the tile loop leave through
// `stopped`, which is not "the block ended": no tile behind the one that holds the stop is staged or walked -- the work is the target's,
// not the block's.  The walk (lz4_seq_walk.h, unchanged) still covers the WHOLE tile that holds the stop before a chunk runs: if it finds
// no chain in the bytes behind the stop (X_ERR), the block is handed back like any irregular one, and lz4_decompress_form_kernel
// (lz4_decompress.hip), which never looks behind the stop, decides it -- correct, and slower for that block only.  Nothing is stored at or
// behind out + target: the window is written back in whole 16-byte units below OP and byte by byte up to OP, and OP never passes the target.
// PARTIAL with DICT (lz4flex_decompress_batch_partial_shared_dict / _dict_set; PARTIAL with OneDict / DictSetArgs): Dec<G, true,
// true>.  The two forms compose with three adjustments.  (1) Positions are virtual, so the crossing sequence's offset check is
// offset > OP - lo(), as in exact_seq; its copies (coop_match / big_match: vp, vbyte, pos_copy) pick their path by the CLIPPED length.
// (2) The target is biased by PV like a capacity -- but a capacity that does not fit the position space may be cut (the block then ends
// in the second pass as OutputTooSmall or decodes), a target may not: cut, it would be reached, and the decode would stop early with
// status 0.  Such a target becomes one no position reaches; a block that really needs positions beyond POS_LIMIT is handed back by the
// position checks.  The "nothing is asked for" exit tests the caller's target, before the bias.  (3) setup_chunk's cut and its
// capacity check both compare with D.cap - op, biased on both sides; the OffsetOutOfBounds ballot (dm - lo()) stays behind the cut, so
// an offset that reaches in front of the dictionary in a sequence behind the stop is no error.  The strict sink holds as it does
// without a dictionary: F starts at PV, a multiple of 16, write_back's units lie below OP & ~15 in virtual positions, and OP never
// passes the biased target.  A block of a set without a dictionary has PV = LO = 0 and decodes exactly as the plain partial form.
// LDS per wavefront: token list 2 560 + tile 4 080 + window 3 584 + 16 = 10 240 bytes: 16 wavefronts per CU (4 096 blocks are one round of
// wavefronts; 8 KiB windows -- 11 per CU, a fifth of the far matches -- were a quarter slower: DESIGN.md 5.2, profiles/r06_seq_decoder.txt).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4_device.h"
#include "lz4_seq_walk.h"

namespace lz4flex_dev {
namespace sq {

using namespace sw;      // the walk, its geometry and the lane / LDS helpers

#ifndef LZ4S_R
#define LZ4S_R 3584
#endif
#ifndef LZ4S_KEEP
#define LZ4S_KEEP 1280
#endif
constexpr uint32_t LITMAX = 64u;             // literal run a lane copies itself
constexpr uint32_t FARMAX = 64u;             // match from the written-back output a lane copies itself
constexpr uint32_t BIGRUN = 1024u;           // literal runs / matches from here on go memory to memory (exact_seq)
// LDS: [token list | tile | window | scratch 16]
constexpr uint32_t LDS_WIN = LDS_TILE + TILE_LDS;
static_assert(PT + 1u + LITMAX + 16u <= PT + TMARGIN && PT + 1u + LITMAX + 8u <= PT + TMARGIN, "a lane's literals and offset lie inside the staged bytes");

template <uint32_t R_, uint32_t KEEP_>
struct Geo {
    static constexpr uint32_t R = R_;                              // window bytes
    static constexpr uint32_t KEEP = KEEP_;                        // history a slide keeps
    static constexpr uint32_t BUDGET = (R_ - KEEP_ - 64u) / 2u;    // output bytes of one chunk (two chunks are in flight) / of one cooperative piece
    static constexpr uint32_t SCRATCH = LDS_WIN + R_;              // 16 bytes behind the window: where a lane's 16-byte source read may end, and where the
    static constexpr uint32_t LDS = LDS_WIN + R_ + 16u;            // later rounds' writes of the wrong size class go (29 x 512 bytes: 11 wavefronts per CU)
    static_assert(R_ >= 1024u + 1040u + 16u, "the window holds a long run's extended period");
};

#ifdef LZ4S_PROF      // tools: cycles of every wavefront per phase -> g_sq_prof[0..15], event counts in [16..31]
__device__ unsigned long long g_sq_prof[32];
struct Prof { uint64_t c[32]; uint64_t t; };
#define SQ_PROF_ARG , Prof& P
#define SQ_PROF_PASS , P
#define SQ_TICK(i) { const uint64_t t_ = __builtin_readcyclecounter(); P.c[i] += t_ - P.t; P.t = t_; }
#define SQ_COUNT(i, n) { P.c[i] += (uint64_t)(n); }
#else
#define SQ_PROF_ARG
#define SQ_PROF_PASS
#define SQ_TICK(i)
#define SQ_COUNT(i, n)
#endif

__device__ __forceinline__ u32x4 lds_rd16(uint32_t a) { u32x4 v; __builtin_memcpy(&v, (const void*)L8(a), 16); return v; }
__device__ __forceinline__ void lds_wr8(uint32_t a, uint32_t lo, uint32_t hi) { const u32x2 v = {lo, hi}; __builtin_memcpy((void*)L8(a), &v, 8); }
__device__ __forceinline__ void lds_wr1(uint32_t a, uint32_t v) { *L8(a) = (uint8_t)v; }

// n (1..16) bytes of v to LDS, exactly (the write_exact16 of the wave decoder this kernel replaced)
__device__ __forceinline__ void write_exact16(uint32_t dst, const u32x4& v, uint32_t n) {
    if (n >= 16u) { lds_wr16(dst, v); return; }
    const bool n8 = (n & 8u) != 0u, n4 = (n & 4u) != 0u, n2 = (n & 2u) != 0u;
    const uint32_t w4 = n8 ? v.z : v.x;                               // the dword at byte offset (n & 8)
    const uint32_t wq = n8 ? (n4 ? v.w : v.z) : (n4 ? v.y : v.x);     // the dword at byte offset (n & 12)
    if (n8) lds_wr8(dst, v.x, v.y);
    if (n4) lds_wr4(dst + (n & 8u), w4);
    if (n2) lds_wr2(dst + (n & 12u), wq);
    if (n & 1u) lds_wr1(dst + (n & 14u), wq >> (n2 ? 16 : 0));
}

// DICT (lz4flex_decompress_batch_shared_dict): ONE external dictionary for every block of the batch, decoded as prefix mode decodes a
// prefix -- but the prefix lives in another buffer.  Positions are VIRTUAL: with dl = min(dict_len, 65 536) (an offset is at most
// 65 535) and PV = dl rounded up to 16, positions [PV - dl, PV) are the dictionary's last dl bytes, PV + k is byte k of the block's
// output, positions below LO = PV - dl do not exist.  `out` and `dv` are both biased by -PV: a position p >= PV is out[p] (every
// store: F starts at PV, a multiple of 16, so write_back's units lie where they lie without a dictionary and none begins in front of
// the sink), a position in [LO, PV) is dv[p] (loads only).  A 16-byte load that straddles PV is put together byte by byte.
template <class G, bool DICT = false, bool PARTIAL = false>
struct Dec {
    const g_u8* in;
    g_u8* out;
    uint32_t ilen, cap, lane;
    uint32_t OP;         // bytes produced
    uint32_t W0;         // the window holds [W0, OP), W0 a multiple of 16
    uint32_t F;          // bytes written back, a multiple of 16 (W0 <= F)
    const g_u8* dv;      // DICT: the dictionary's end - PV
    uint32_t PV, LO;     // DICT: the output's first position; the oldest position there is

    __device__ __forceinline__ uint32_t lo() const { return DICT ? LO : 0u; }
    // DICT: where the byte of position p (>= LO; written back if >= PV) lies, and the byte (0 in front of LO)
    __device__ __forceinline__ const g_u8* vp(uint32_t p) const { return (p < PV ? dv : (const g_u8*)out) + p; }
    __device__ __forceinline__ uint32_t vbyte(uint32_t p) const { return p >= LO ? (uint32_t)*vp(p) : 0u; }
    // DICT: the 16 bytes at position p, of which those in front of `lim` exist
    __device__ __forceinline__ u32x4 vload16(uint32_t p, uint32_t lim) const {
        u32x4 v;
        if (p >= LO && p + 16u <= lim && (p >= PV || p + 16u <= PV)) __builtin_memcpy(&v, (const void*)vp(p), 16);
        else {
            uint32_t wv[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (uint32_t k = 0u; k < 16u; ++k) if (p + k < lim) wv[k >> 2] |= vbyte(p + k) << (8u * (k & 3u));
            v = u32x4{wv[0], wv[1], wv[2], wv[3]};
        }
        return v;
    }

    // window -> output, whole 16-byte units of [F, op)
    __device__ __forceinline__ void write_back(uint32_t op) {
        const uint32_t lim = op & ~15u;
        for (uint32_t q0 = F; q0 < lim; q0 += 1024u) {         // (uniform trip counts, the lanes' share inside: a loop that lanes leave at different
            const uint32_t q = q0 + 16u * lane;                 //  times makes the compiler take every value merged behind it for divergent)
            if (q < lim) {
                const u32x4 v = lds_rd16(LDS_WIN + (q - W0));
                __builtin_memcpy((void*)(out + q), &v, 16);
            }
            SW_JOIN();
        }
        F = lim;
    }
    // make room for `need` (<= 2 BUDGET) more bytes behind op: write back, move the last KEEP bytes to the window's start
    __device__ __forceinline__ void ensure(uint32_t op, uint32_t need) {
        if (op - W0 + need <= G::R) return;
        write_back(op);
        const uint32_t nw = (op - G::KEEP) & ~15u;           // (op - W0 > KEEP here: need <= R - KEEP - 64)
        const uint32_t S = nw - W0, n = op - nw;
        for (uint32_t i0 = 0u; i0 < n; i0 += 1024u) {        // a lower iteration never writes what a higher one reads (S >= 0); within one, reads precede writes
            const uint32_t i = i0 + 16u * lane;
            if (i < n) {
                const u32x4 v = lds_rd16(LDS_WIN + S + i);
                lds_wr16(LDS_WIN + i, v);
            }
            SW_JOIN();
        }
        W0 = nw;
    }
    // everything produced so far, the last odd bytes too
    __device__ __forceinline__ void flush_all() {
        write_back(OP);
        if (F + lane < OP) out[F + lane] = *L8(LDS_WIN + F + lane - W0);
        SW_JOIN();
    }
    __device__ __forceinline__ void finish() {
        flush_all();
        F = OP;
    }
    // ---- runs of BIGRUN bytes or more go memory to memory, 16 bytes per lane, and the window is read back behind them ----------------
    // the window = the last KEEP bytes of the output, from memory (this wavefront's own stores: one CU, one L1 -- coherent in program order)
    __device__ __forceinline__ void reload_window() {
        W0 = OP > G::KEEP ? (OP - G::KEEP) & ~15u : 0u;
        const uint32_t n = OP - W0;
        for (uint32_t i0 = 0u; i0 < n; i0 += 1024u) {
            const uint32_t i = i0 + 16u * lane;
            if (i < n) {
                u32x4 v = {0u, 0u, 0u, 0u};
                if constexpr (DICT) v = vload16(W0 + i, OP);
                else if (W0 + i + 16u <= OP) __builtin_memcpy(&v, (const void*)(out + W0 + i), 16);
                else {
                    uint32_t wv[4] = {0u, 0u, 0u, 0u};
                    for (uint32_t k = 0u; k < 16u; ++k) if (W0 + i + k < OP) wv[k >> 2] |= (uint32_t)out[W0 + i + k] << (8u * (k & 3u));
                    v = u32x4{wv[0], wv[1], wv[2], wv[3]};
                }
                lds_wr16(LDS_WIN + i, v);
            }
            SW_JOIN();
        }
        F = OP & ~15u;
    }
    // n bytes from memory at `from` to the output at OP, 1 KiB per step in order (a step's source may be an earlier step's destination)
    __device__ __forceinline__ void mem_copy(const g_u8* from, uint32_t n) {
        for (uint32_t i0 = 0u; i0 < n; i0 += 1024u) {
            const uint32_t i = i0 + 16u * lane;
            if (i + 16u <= n) {
                u32x4 v;
                __builtin_memcpy(&v, (const void*)(from + i), 16);
                __builtin_memcpy((void*)(out + OP + i), &v, 16);
            } else if (i < n) {
                for (uint32_t k = i; k < n; ++k) out[OP + k] = from[k];
            }
            SW_JOIN();
        }
    }
    // DICT: the same from position sp (a match's source: in the dictionary, in the output, or across both)
    __device__ __forceinline__ void pos_copy(uint32_t sp, uint32_t n) {
        for (uint32_t i0 = 0u; i0 < n; i0 += 1024u) {
            const uint32_t i = i0 + 16u * lane;
            if (i + 16u <= n) {
                const u32x4 v = vload16(sp + i, sp + n);
                __builtin_memcpy((void*)(out + OP + i), &v, 16);
            } else if (i < n) {
                for (uint32_t k = i; k < n; ++k) out[OP + k] = (uint8_t)vbyte(sp + k);
            }
            SW_JOIN();
        }
    }
    __device__ __forceinline__ uint32_t mod_small(uint32_t i, uint32_t m, float rcp) {      // i mod m, i < 2^22, rcp = 1 / m
        const uint32_t q = (uint32_t)((float)i * rcp);
        uint32_t r = i - q * m;                                    // q is off by at most one either way
        r = (int32_t)r < 0 ? r + m : r;
        return r >= m ? r - m : r;
    }
    __device__ void big_literals(uint32_t src, uint32_t n) {
        flush_all();
        mem_copy(in + src, n);
        OP += n;
        reload_window();
    }
    // a long match.  offset >= 1024: a step's source lies in front of the step: memory to memory.  Else the periodic form
    // out[d + i] = out[d - offset + i mod offset] (decompress.rs:57-82, decompress_safe.rs:301-318; offset 1 = a run of one byte, :311-313):
    // the period, repeated to 1 KiB + 16 + offset bytes in the (flushed) window's place, is what every step stores a kibibyte of
    __device__ void big_match(uint32_t offset, uint32_t n) {
        flush_all();
        if (offset >= 1024u) {
            if constexpr (DICT) pos_copy(OP - offset, n);
            else mem_copy(out + OP - offset, n);
        } else {
            const float rcp = 1.0f / (float)offset;
            const uint32_t el = offset + 1040u;
            for (uint32_t k0 = 0u; k0 < el; k0 += 64u) {
                const uint32_t k = k0 + lane;
                if constexpr (DICT) { if (k < el) *L8(LDS_WIN + k) = (uint8_t)vbyte(OP - offset + mod_small(k, offset, rcp)); }
                else if (k < el) *L8(LDS_WIN + k) = out[OP - offset + mod_small(k, offset, rcp)];
                SW_JOIN();
            }
            uint32_t ph = 0u;                                      // i0 mod offset
            const uint32_t adv = mod_small(1024u, offset, rcp);
            for (uint32_t i0 = 0u; i0 < n; i0 += 1024u) {
                const uint32_t i = i0 + 16u * lane;
                if (i < n) {
                    const u32x4 v = lds_rd16(LDS_WIN + ph + 16u * lane);
                    if (i + 16u <= n) __builtin_memcpy((void*)(out + OP + i), &v, 16);
                    else {
                        const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
                        for (uint32_t k = 0u; i + k < n; ++k) out[OP + i + k] = (uint8_t)(wv[k >> 2] >> (8u * (k & 3u)));
                    }
                }
                SW_JOIN();
                ph += adv;
                ph = ph >= offset ? ph - offset : ph;
            }
        }
        OP += n;
        reload_window();
    }
    // literals of any length from the compressed stream, whole wavefront, <= BUDGET bytes per piece
    __device__ __forceinline__ void coop_literals(uint32_t src, uint32_t n) {
        if (n >= BIGRUN) { big_literals(src, n); return; }
        for (uint32_t c = 0u; c < n; c += G::BUDGET) {
            const uint32_t m = n - c < G::BUDGET ? n - c : G::BUDGET;
            ensure(OP, m);
            for (uint32_t i0 = 0u; i0 < m; i0 += 64u) {
                const uint32_t i = i0 + lane;
                if (i < m) *L8(LDS_WIN + OP - W0 + i) = in[src + c + i];
                SW_JOIN();
            }
            OP += m;
        }
    }
    // a match of any offset / length, whole wavefront, 64 bytes per step.  Source bytes from the window when it holds them, else
    // from the output written back earlier.  offset < 64: the periodic form out[d + i] = out[d - offset + i mod offset]
    // (decompress.rs:57-82, decompress_safe.rs:301-318), which only reads bytes in front of the match.
    __device__ __forceinline__ void coop_match(uint32_t offset, uint32_t n) {
        if (n >= BIGRUN) { big_match(offset, n); return; }
        const float rcp = offset < 64u ? 1.0f / (float)offset : 0.0f;
        for (uint32_t c = 0u; c < n; c += G::BUDGET) {
            const uint32_t m = n - c < G::BUDGET ? n - c : G::BUDGET;
            ensure(OP, m);
            const uint32_t d = OP, src = d - offset;
            for (uint32_t s0 = 0u; s0 < m; s0 += 64u) {
                const uint32_t i = s0 + lane;
                if (i < m) {
                    uint32_t si = i;
                    if (offset < 64u) {
                        const uint32_t q = (uint32_t)((float)i * rcp);
                        uint32_t r = i - q * offset;                  // q is off by at most one either way
                        r = (int32_t)r < 0 ? r + offset : r;
                        r = r >= offset ? r - offset : r;
                        si = r;
                    }
                    const uint32_t ps = src + si;
                    const uint8_t byte = ps >= W0 ? *L8(LDS_WIN + ps - W0) : (DICT ? *vp(ps) : out[ps]);
                    *L8(LDS_WIN + d - W0 + i) = byte;
                }
                SW_JOIN();
            }
            OP += m;
        }
    }
    // One sequence of any shape at `ip`, by the whole wavefront, with the reference's checks (decompress.rs:334-443; any violation ->
    // false: the reference-order kernel decodes the block again and names the error).  done: the block ended here.
    __device__ bool exact_seq(uint32_t ip, bool& done) {
        const uint32_t t = uni(in[ip]);
        ip += 1u;
        uint32_t lit = t >> 4;
        if (lit == 15u) {
            for (;;) {
                if (ip >= ilen) return false;
                const uint32_t b = uni(in[ip]);
                ip += 1u;
                lit += b;
                if (lit > 0x7FFFFFFFu) return false;      // (a 32-bit sum must not wrap: the reference counts in usize)
                if (b != 255u) break;
            }
        }
        if (lit > ilen - ip || lit > cap - OP || OP + lit > POS_LIMIT) return false;
        coop_literals(ip, lit);
        ip += lit;
        if (ip >= ilen) { done = true; return true; }
        if (ilen - ip < 2u) return false;
        const uint32_t offset = uni((uint32_t)in[ip] | ((uint32_t)in[ip + 1u] << 8));
        ip += 2u;
        if (offset == 0u) return false;
        uint32_t ml = 4u + (t & 15u);
        if (ml == 19u) {
            for (;;) {
                if (ip >= ilen) return false;
                const uint32_t b = uni(in[ip]);
                ip += 1u;
                ml += b;
                if (ml > 0x7FFFFFFFu) return false;
                if (b != 255u) break;
            }
        }
        if (offset > OP - lo() || ml > cap - OP || OP + ml > POS_LIMIT) return false;
        coop_match(offset, ml);
        if (ip >= ilen) return false;              // a match is always followed by another token (decompress.rs:439-443)
        return true;
    }
    // PARTIAL: the same with `cap` as the target (OP < cap on entry).  The lengths are checked in full, in the reference's order, and
    // copied clipped to cap - OP; a copy that reaches the target ends the decode there (SEQ_STOP) and nothing behind it is looked at.
    // (the outcome is a value, not two flags by reference: flags whose address is taken by a real call live in scratch memory)
    enum : uint32_t { SEQ_BAD = 0u, SEQ_MORE = 1u, SEQ_END = 2u, SEQ_STOP = 3u };
    __device__ uint32_t exact_seq_partial(uint32_t ip) {
        const uint32_t t = uni(in[ip]);
        ip += 1u;
        uint32_t lit = t >> 4;
        if (lit == 15u) {
            for (;;) {
                if (ip >= ilen) return SEQ_BAD;
                const uint32_t b = uni(in[ip]);
                ip += 1u;
                lit += b;
                if (lit > 0x7FFFFFFFu) return SEQ_BAD;
                if (b != 255u) break;
            }
        }
        if (lit > ilen - ip) return SEQ_BAD;
        {
            const uint32_t c = lit < cap - OP ? lit : cap - OP;
            if (OP + c > POS_LIMIT) return SEQ_BAD;
            coop_literals(ip, c);
        }
        if (OP >= cap) return SEQ_STOP;
        ip += lit;
        if (ip >= ilen) return SEQ_END;
        if (ilen - ip < 2u) return SEQ_BAD;
        const uint32_t offset = uni((uint32_t)in[ip] | ((uint32_t)in[ip + 1u] << 8));
        ip += 2u;
        if (offset == 0u) return SEQ_BAD;
        uint32_t ml = 4u + (t & 15u);
        if (ml == 19u) {
            for (;;) {
                if (ip >= ilen) return SEQ_BAD;
                const uint32_t b = uni(in[ip]);
                ip += 1u;
                ml += b;
                if (ml > 0x7FFFFFFFu) return SEQ_BAD;
                if (b != 255u) break;
            }
        }
        if (offset > OP - lo()) return SEQ_BAD;
        {
            const uint32_t c = ml < cap - OP ? ml : cap - OP;
            if (OP + c > POS_LIMIT) return SEQ_BAD;
            coop_match(offset, c);
        }
        if (OP >= cap) return SEQ_STOP;      // (a match that ends at the target is not asked for the token behind it)
        if (ip >= ilen) return SEQ_BAD;
        return SEQ_MORE;
    }
};

// A chunk: up to 64 consecutive sequences of the tile's token list, lane = sequence, placed but not yet copied
struct Chunk {
    uint32_t lit, ml, dst, src, lsr;    // per lane: lengths, output position of the literals, source position of the match, literals' position relative to t0
    u32x4 f0, f1, f2, f3;               // a far match's source bytes (requested at set-up, used a chunk later)
    uint64_t act, haslit, near, far;    // lanes: in the chunk; with literals; match from the window; match from the written-back output
    uint32_t nact, T, tp0;              // sequences, output bytes; nact == 0: the sequence at tp0 (relative to t0) is executed alone by the wavefront
    bool last;                          // the block's last sequence is the chunk's last
};

// Set-up of the chunk that starts at sequence sidx with `op` bytes in front of it -- of which the last `pending` are still being
// produced by the chunk before (room for both is made here: a slide never moves a placed chunk).  false: the block is irregular.
// PARTIAL (op < D.cap, the target): the chunk ends in front of the first sequence that reaches or crosses the target.
template <class G, bool DICT, bool PARTIAL>
__device__ __forceinline__ bool setup_chunk(Dec<G, DICT, PARTIAL>& D, uint32_t t0, uint32_t n_tile, uint32_t sidx, uint32_t op, uint32_t pending, Chunk& C) {
    const uint32_t lane = D.lane;
    const uint32_t ilr = D.ilen - t0;                          // the block's end, relative to t0
    const uint32_t nrem = n_tile - sidx;
    // ---- token, lengths, offset; a literal run of more than LITMAX bytes is not a lane's work: exact_seq --------------------------
    const Token t = decode_token<LITMAX>(sidx + (lane < nrem ? lane : nrem - 1u), ilr);
    const uint32_t tpr = t.tpr, lit = t.lit, lsr = t.lsr, lend = t.lend, off = t.off, e2 = t.e2, mlx = t.mlx, nxt = t.nxt;
    const bool m15 = t.m15;
    const uint64_t biglit = t.biglit, lastm = t.lastm;
    const uint64_t errm = ballot(lend > ilr) |                                                           // :346-348
                          (~lastm & (ballot(lend + 2u > ilr) | ballot(nxt >= ilr) | ballot(off == 0u))); // :373-375, :439-443, :168-173
    const uint64_t bigm = biglit | (~lastm & (ballot(m15 && e2 == 255u) | ballot(off < mlx)));           // more length bytes; a match that reads its own output
    const uint32_t ml = lanes(lastm) ? 0u : mlx;
    // ---- the chunk: up to the first sequence that is not a lane's work, and at most BUDGET bytes ------------------------------
    uint32_t nact = nrem < 64u ? nrem : 64u;
    {
        const uint64_t bm = bigm & low_mask(nact);
        if (bm != 0ull) nact = ctz64(bm);
    }
    const uint32_t u = lanes(low_mask(nact)) ? lit + ml : 0u;
    const uint32_t incl = wave_incl_add(u);
    {
        const uint64_t over = ballot(incl > G::BUDGET) & low_mask(nact);
        if (over != 0ull) nact = ctz64(over);
    }
    if constexpr (PARTIAL) {
        // the sequences that end STRICTLY before the target (one that ends at it stops the decode and must not get the "followed by a
        // token" check errm carries for its lane): the cut comes before errm is looked at -- what lies behind the stop is no error
        const uint64_t reach = ballot(incl >= D.cap - op) & low_mask(nact);
        if (reach != 0ull) nact = ctz64(reach);
    }
    uint32_t T = nact != 0u ? rdlane(incl, nact - 1u) : 0u;
    C.tp0 = rdlane(tpr, 0u);
    if (nact != 0u) {
        if ((errm & low_mask(nact)) != 0ull) return false;
        if (T > D.cap - op || op + T > POS_LIMIT) return false;    // OutputTooSmall (:349-356, :403-408): named by the reference-order kernel
        D.write_back(op - pending);                            // (every chunk: a source that leaves the window has to be in memory)
        D.ensure(op - pending, pending + T);
    }
    const uint32_t dst = op + incl - u, dm = dst + lit;
    const uint32_t src = dm - off;
    uint64_t am = low_mask(nact);
    const uint64_t hasm = ~lastm;
    if ((ballot(off > dm - D.lo()) & hasm & am) != 0ull) return false;  // OffsetOutOfBounds (:286-289, :398-402)
    // a source in front of the window comes from the written-back output: all of it has to be there, and short enough for a lane.
    // "The window" is what the NEXT chunk's set-up will have left of it when this chunk is copied: a slide keeps KEEP bytes in front
    // of the chunk that is pending then -- this one
    const uint32_t near_lo = op > G::KEEP && op - G::KEEP > D.W0 ? op - G::KEEP : D.W0;
    const uint64_t farm = ballot(src < near_lo) & hasm;
    {
        uint64_t fbig = farm & am & (ballot(src + ml > D.F) | ballot(ml > FARMAX));
        // DICT: a far source whose 16-byte loads could cross from the dictionary into the output is exact_seq's (byte loads)
        if constexpr (DICT) fbig |= farm & am & ballot(src < D.PV && src + FARMAX > D.PV);
        if (fbig != 0ull) { nact = ctz64(fbig); am = low_mask(nact); T = nact != 0u ? rdlane(incl, nact - 1u) : 0u; }
    }
    C.lit = lit; C.ml = ml; C.dst = dst; C.src = src; C.lsr = lsr;
    C.nact = nact; C.T = T;
    C.act = am;
    C.haslit = ballot(lit != 0u) & am;
    C.far = farm & am;
    C.near = hasm & am & ~farm;
    C.last = nact != 0u && ((lastm >> (nact - 1u)) & 1ull) != 0ull;
    // ---- far sources: requested now, used a chunk later --------------------------------------------------------------------------
    C.f0 = u32x4{0u, 0u, 0u, 0u}; C.f1 = C.f0; C.f2 = C.f0; C.f3 = C.f0;
    if (lanes(C.far)) {
        const g_u8* fs = DICT ? D.vp(src) : D.out + src;       // (DICT: [src, src + FARMAX) lies on one side of PV)
        __builtin_memcpy(&C.f0, (const void*)fs, 16);
        if (ml > 16u) __builtin_memcpy(&C.f1, (const void*)(fs + ml - 16u), 16);
        if (ml > 32u) __builtin_memcpy(&C.f2, (const void*)(fs + 16u), 16);
        if (ml > 48u) __builtin_memcpy(&C.f3, (const void*)(fs + 32u), 16);
    }
    SW_JOIN();
    return true;
}

// What a lane needs to copy its n bytes (1 <= n) from LDS address s to LDS address d: the addresses of the LAST 16 bytes on both sides
// and the lanes of every size class.  One 16-byte read (16 bytes and more: a second one, of the LAST 16 bytes) and two overlapping
// writes of the size class; more than 32 bytes: the pieces between them.  Source and destination do not
// overlap.  Computed once per chunk; the rounds only AND the classes with their ready lanes.
struct CopyPlan {
    uint32_t s, d, s2, d2, n;
    uint64_t c16, c8, c4, c2, c1, gt32;       // n >= 16; 8..15; 4..7; 2..3; 1; n > 32
};
template <bool SMALL>
__device__ __forceinline__ CopyPlan plan_copy(uint32_t s, uint32_t d, uint32_t n) {
    CopyPlan P;
    P.s = s; P.d = d; P.n = n; P.s2 = s + n - 16u; P.d2 = d + n - 16u;
    const uint64_t ge16 = ballot(n >= 16u), ge8 = ballot(n >= 8u);
    P.c16 = ge16; P.c8 = ge8 & ~ge16; P.gt32 = ballot(n > 32u);
    if (SMALL) {
        const uint64_t ge4 = ballot(n >= 4u), ge2 = ballot(n >= 2u);
        P.c4 = ge4 & ~ge8; P.c2 = ge2 & ~ge4; P.c1 = ~ge2;
    } else { P.c4 = ~ge8; P.c2 = 0ull; P.c1 = 0ull; }
    return P;
}
template <bool SMALL>
__device__ __forceinline__ void lane_copy(const CopyPlan& P, uint64_t m) {
    u32x4 r1;
    if (lanes(m)) r1 = lds_rd16(P.s);
    // 16 bytes and more: the last 16 bytes are a second read; less: they are bytes of the first (an LDS instruction costs the CU's one LDS
    // pipe whatever the number of lanes, a handful of vector instructions costs one of four SIMDs)
    if (lanes(m & P.c16)) { const u32x4 r2 = lds_rd16(P.s2); lds_wr16(P.d, r1); lds_wr16(P.d2, r2); }
    if (lanes(m & P.c8)) {                                   // n = 8 .. 15: bytes [n - 8, n) of r1
        const uint32_t k = P.n - 8u;
        const bool lo4 = k < 4u;
        const uint32_t a = lo4 ? r1.x : r1.y, b = lo4 ? r1.y : r1.z, c = lo4 ? r1.z : r1.w;
        lds_wr8(P.d, r1.x, r1.y);
        lds_wr8(P.d2 + 8u, __builtin_amdgcn_alignbyte(b, a, k & 3u), __builtin_amdgcn_alignbyte(c, b, k & 3u));
    }
    if (lanes(m & P.c4)) { lds_wr4(P.d, r1.x); lds_wr4(P.d2 + 12u, __builtin_amdgcn_alignbyte(r1.y, r1.x, P.n & 3u)); }     // n = 4 .. 7: bytes [n - 4, n)
    if (SMALL) {
        if (lanes(m & P.c2)) { lds_wr2(P.d, r1.x); lds_wr2(P.d2 + 14u, r1.x >> (8u * (P.n - 2u))); }                          // n = 2, 3
        if (lanes(m & P.c1)) lds_wr1(P.d, r1.x);
    }
    SW_JOIN();
    uint64_t more = m & P.gt32;
    for (uint32_t p = 16u; more != 0ull; p += 16u) {
        if (lanes(more)) { const u32x4 r = lds_rd16(P.s + p); lds_wr16(P.d + p, r); }
        SW_JOIN();
        more &= ballot(p + 32u < P.n);                        // the next piece, at p + 16, begins in front of the last one's start: p + 16 < n - 16
    }
}

// The copies of a placed chunk (decompress.rs:276-280, 314-325, 357-361, 410-437).
template <class G, bool DICT, bool PARTIAL>
__device__ __forceinline__ void exec_chunk(Dec<G, DICT, PARTIAL>& D, const Chunk& C SQ_PROF_ARG) {
    const uint32_t wb = LDS_WIN - D.W0;                        // window address of output position 0
    const uint32_t wl = wb + C.dst, wm = wl + C.lit;
    // ---- literals: 16 bytes per access, exact length ---------------------------------------------------------------------------
    if (C.haslit != 0ull) { const CopyPlan L = plan_copy<true>(LDS_TILE + TPAD + C.lsr, wl, C.lit); lane_copy<true>(L, C.haslit); }
    SQ_TICK(6)
    // ---- far matches: the bytes requested at set-up -------------------------------------------------------------------------------
    if (C.far != 0ull) {
        if (lanes(C.far)) {
            if (C.ml <= 16u) write_exact16(wm, C.f0, C.ml);
            else {
                lds_wr16(wm, C.f0);
                if (C.ml > 32u) lds_wr16(wm + 16u, C.f2);
                if (C.ml > 48u) lds_wr16(wm + 32u, C.f3);
                lds_wr16(wm + C.ml - 16u, C.f1);
            }
        }
        SW_JOIN();
    }
    SQ_TICK(7) SQ_COUNT(17, 1) SQ_COUNT(20, C.nact) SQ_COUNT(23, __builtin_popcountll(C.far)) SQ_COUNT(24, __builtin_popcountll(C.near))
    // ---- matches inside the window, in rounds: ready = every sequence that starts before the source's end is done ----------------
    uint64_t todo = C.near;
    const CopyPlan M = plan_copy<false>(wb + C.src, wm, C.ml);
    const uint32_t s1 = C.src + C.ml;
    if (todo != 0ull) {
        // the first round: most of the chunk's matches (every source in front of the chunk)
        const uint32_t dp = ctz64(todo);                      // every lane below dp is done: all bytes in front of its sequence are final
        const uint32_t S = rdlane(C.dst, dp);
        const uint64_t rm = todo & (ballot(s1 <= S) | (1ull << dp));
        lane_copy<false>(M, rm);
        todo &= ~rm;
        SQ_COUNT(18, 1)
#ifdef LZ4S_EXP_NOROUNDS      // timing experiments only (wrong bytes): the first round alone
        todo = 0ull;
#endif
    }
    while (todo != 0ull) {
        const uint32_t dp = ctz64(todo);
        const uint32_t S = rdlane(C.dst, dp);
        const uint64_t rm = todo & (ballot(s1 <= S) | (1ull << dp));
        lane_copy<false>(M, rm);
        todo &= ~rm;
        SQ_COUNT(18, 1)
#ifdef LZ4S_EXP_NOROUNDS      // timing experiments only (wrong bytes): the first round alone
        todo = 0ull;
#endif
    }
    SQ_TICK(8)
}

// The chunks of one tile: sequences [0, n_tile) of the token list.  Two chunks are in flight: the next one is set up (token decode,
// placement, checks, room in the window, requests for far sources) before the current one is copied.  false: the block is irregular.
// PARTIAL: `stopped` = the target is reached (anywhere in the tile: the sequences behind the stop are not looked at), else as `done`.
template <class G, bool DICT, bool PARTIAL>
__device__ __forceinline__ bool run_chunks(Dec<G, DICT, PARTIAL>& D, uint32_t t0, uint32_t n_tile, bool& done, [[maybe_unused]] bool& stopped SQ_PROF_ARG) {
    uint32_t sidx = 0u;
    Chunk C;
    if (!setup_chunk<G, DICT, PARTIAL>(D, t0, n_tile, 0u, D.OP, 0u, C)) return false;
    SQ_TICK(4)
    for (;;) {
        if (C.nact == 0u) {                                    // the sequence alone, by the whole wavefront
            if constexpr (PARTIAL) {
                const uint32_t r = D.exact_seq_partial(t0 + C.tp0);
                if (r == D.SEQ_BAD) return false;
                if (r == D.SEQ_STOP) { stopped = true; return true; }
                done = r == D.SEQ_END;
            } else if (!D.exact_seq(t0 + C.tp0, done)) return false;
            sidx += 1u;
            SQ_TICK(9) SQ_COUNT(19, 1)
            if (done) return sidx == n_tile;
            if (sidx >= n_tile) return true;
            if (!setup_chunk<G, DICT, PARTIAL>(D, t0, n_tile, sidx, D.OP, 0u, C)) return false;
            SQ_TICK(4)
            continue;
        }
        const uint32_t nsidx = sidx + C.nact, nop = D.OP + C.T;
        const bool have_next = nsidx < n_tile && !C.last;
        Chunk N;
        N.nact = 0u; N.T = 0u; N.tp0 = 0u; N.last = false; N.act = 0ull; N.haslit = 0ull; N.near = 0ull; N.far = 0ull;
        N.lit = 0u; N.ml = 0u; N.dst = 0u; N.src = 0u; N.lsr = 0u;
        N.f0 = u32x4{0u, 0u, 0u, 0u}; N.f1 = N.f0; N.f2 = N.f0; N.f3 = N.f0;
        if (have_next) { if (!setup_chunk<G, DICT, PARTIAL>(D, t0, n_tile, nsidx, nop, C.T, N)) return false; }
        SQ_TICK(4)
#ifndef LZ4S_EXP_NOEXEC         // timing experiments only (wrong bytes): chunks are placed, nothing is copied
        exec_chunk<G, DICT, PARTIAL>(D, C SQ_PROF_PASS);
#endif
        D.OP = nop;
        sidx = nsidx;
        if (C.last) { done = true; return sidx == n_tile; }
        if (!have_next) return true;
        C = N;
    }
}

#ifdef LZ4S_WAVES      // tools: wavefronts per SIMD the register allocation aims at (the kernel's 116 VGPRs allow 4: 16 per CU)
#define LZ4S_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(LZ4S_WAVES, LZ4S_WAVES)))
#else
#define LZ4S_WAVES_ATTR
#endif
// SRC: where the blocks' dictionaries come from (lz4_device.h).  OneDict: none has a prefix.  DictSetArgs: block b has the dictionary its
// id names in a prepared set -- or none (dl = 0, so PV = LO = 0: the block decodes as it does without the dictionary form), or a refused
// id.  PARTIAL: no prefix, and a.out_cap[b] is block b's TARGET (see the head of the file).
template <class G, class SRC, bool PARTIAL>
__global__ void __launch_bounds__(64) LZ4S_WAVES_ATTR lz4_decompress_seq_kernel(DecompressArgs a, int32_t redo_code, SRC src) {
    constexpr bool DICT = !__is_same(SRC, NoDict);
    extern __shared__ __attribute__((aligned(16))) uint8_t seq_lds[];
    const uint32_t lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    if (b >= a.n) return;
    [[maybe_unused]] const uint8_t* dict = nullptr;
    [[maybe_unused]] uint32_t dict_len = 0u;
    if (!dict_find(src, b, dict, dict_len)) {
        if (lane == 0u) {
            a.status[b] = LZ4FLEX_DEV_E_INVALID_ARG;
            a.out_len[b] = 0u;
            if (a.detail) { a.detail[2u * b] = 0u; a.detail[2u * b + 1u] = 0u; }
        }
        return;
    }
    if constexpr (__is_same(SRC, DictSetArgs)) {
        // (the wavefront's one record, said to be uniform: PV / LO / dv below are scalars as they are with the launch's one dictionary)
        const uint64_t dp = (uint64_t)(uintptr_t)dict;
        dict = (const uint8_t*)(uintptr_t)(((uint64_t)uni((uint32_t)(dp >> 32)) << 32) | uni((uint32_t)dp));
        dict_len = uni(dict_len);
    }
    // (every LDS access below goes by byte address from 0: the dynamic segment is the kernel's only LDS)
    if ((uint32_t)(uintptr_t)(lds_u8*)seq_lds != 0u) { if (lane == 0u) { a.status[b] = redo_code; a.out_len[b] = 0u; } return; }
    Dec<G, DICT, PARTIAL> D;
    D.in = (const g_u8*)(a.in_base + a.in_off[b]);
    D.out = (g_u8*)(a.out_base + a.out_off[b]);
    D.ilen = a.in_len[b];
    D.cap = a.out_cap[b];
    [[maybe_unused]] const uint32_t want = D.cap;     // PARTIAL: the caller's target (DICT biases D.cap below)
    D.lane = lane;
    D.OP = 0u; D.W0 = 0u; D.F = 0u;
    D.dv = nullptr; D.PV = 0u; D.LO = 0u;
    // PREFIX mode (out_pos, round 6; decompress_into_with_prefix-like: a Linked frame's block, src/frame/decompress.rs:195-222,280-305): the
    // sink already holds [0, PFX) of the stream, matches may reach into it, and the block's bytes follow at PFX -- for this decoder a source in
    // front of its window is a read of written-back output anyway; the prefix is the same read.  The window starts as the last KEEP bytes
    // of the prefix.  (Not for CHAINED batches: the bytes must be in memory when the launch starts -- a level of chains per launch.)
    uint32_t PFX = 0u;
    if constexpr (DICT) {
        // the dictionary as a VIRTUAL prefix (see Dec): nothing is ever stored at a position below PV -- not into the dictionary every
        // block shares, not in front of out_off -- and the capacity counts from PV (a sink so large that `cap + PV` would pass
        // POS_LIMIT is cut there: a block that needs more is the reference-order kernel's)
        const uint32_t dl = dict_len < 65536u ? dict_len : 65536u;
        PFX = (dl + 15u) & ~15u;
        D.PV = PFX; D.LO = PFX - dl;
        D.dv = (const g_u8*)((uintptr_t)dict + dict_len - PFX);
        D.out = (g_u8*)((uintptr_t)(a.out_base + a.out_off[b]) - PFX);
        // PARTIAL: the target counts from PV too -- and one the position space does not hold is never reached, not cut (head of the file)
        if constexpr (PARTIAL) D.cap = D.cap <= POS_LIMIT - PFX ? D.cap + PFX : 0xFFFFFFFFu;
        else D.cap = (D.cap < POS_LIMIT - PFX ? D.cap : POS_LIMIT - PFX) + PFX;
    } else if constexpr (!PARTIAL) {
        PFX = a.out_pos != nullptr ? uni(a.out_pos[b]) : 0u;
    }
    const uint32_t ilen = D.ilen;
    if constexpr (PARTIAL) {
        // nothing is asked for: nothing is read (an EMPTY block is an error before that, decompress.rs:207-209: handed back below)
        if (want == 0u && ilen != 0u) { if (lane == 0u) { a.status[b] = 0; a.out_len[b] = 0u; } return; }
    }
    bool ok = ilen != 0u && ilen <= POS_LIMIT && PFX <= POS_LIMIT / 2u && D.cap >= PFX, done = false;     // (an empty block: decompress.rs:207-209, the reference-order kernel reports it)
    if (PFX != 0u && ok) { D.OP = PFX; D.reload_window(); }
    uint32_t entry = 0u;
#ifdef LZ4S_PROF
    Prof P;
    for (int i = 0; i < 32; ++i) P.c[i] = 0ull;
    P.t = __builtin_readcyclecounter();
#endif
    if (lane < 4u) lds_wr4(LDS_TILE + 4u * lane, 0u);     // the bytes in front of the first tile
    for (;;) {
        // (loop-carried scalars, said to be uniform: a value merged behind a loop that lanes leave at different times -- the walks -- is
        // divergent to the compiler, and everything computed from it lands in vector registers)
        entry = uni(entry); D.OP = uni(D.OP); D.W0 = uni(D.W0); D.F = uni(D.F);
        if (uni((ok && !done) ? 1u : 0u) == 0u) break;
        const uint32_t t0 = entry & ~15u;
        SQ_TICK(15)
        stage_tile(D.in, ilen, t0, lane);
        SQ_TICK(0) SQ_COUNT(16, 1)
        const uint32_t ilr = ilen - t0;
        const uint32_t entry_r = entry - t0;
        Part s;
        first_walks(D.in, ilen, t0, lane, entry_r, s);
        SQ_TICK(1)
        uint32_t my_entry, rounds;
        const uint32_t tile_exit = settle_chain(D.in, ilen, t0, lane, entry_r, s, my_entry, rounds);
        SQ_TICK(2) SQ_COUNT(21, rounds)
        if (tile_exit == X_ERR) { ok = false; break; }
        const uint32_t n_tile = write_token_list(lane, my_entry, s);
        if (n_tile > POSCAP || n_tile == 0u) { ok = false; break; }
        SQ_TICK(3)
        // ---- the chunks -------------------------------------------------------------------------------------------------------------------
        bool tdone = false;
        [[maybe_unused]] bool stopped = false;
#ifdef LZ4S_EXP_NOCHUNKS       // timing experiments only (no output): the walks and the token list alone
        if (tile_exit >= ilr) { done = true; break; }
        entry = t0 + tile_exit;
        continue;
#endif
        if (!run_chunks<G, DICT, PARTIAL>(D, t0, n_tile, tdone, stopped SQ_PROF_PASS)) { ok = false; break; }
        if constexpr (PARTIAL) { if (stopped) { done = true; break; } }     // the target is reached: no further tile is staged or walked
        if (tdone) { done = true; break; }
        if (tile_exit >= ilr) { ok = false; break; }        // the chain ran out without a last sequence
        entry = t0 + tile_exit;
        // (a long literal run or match length run jumps over tiles: the next tile starts where the chain goes on)
    }
    if (ok && done) {
        SQ_TICK(15)
        D.finish();
        SQ_TICK(10)
#ifdef LZ4S_PROF
        if (lane == 0u) for (int i = 0; i < 32; ++i) if (P.c[i] != 0ull) atomicAdd(&g_sq_prof[i], (unsigned long long)P.c[i]);
#endif
        if (lane == 0u) {
            a.status[b] = 0;
            a.out_len[b] = D.OP - PFX;
            if (a.detail) { a.detail[2u * b] = 0u; a.detail[2u * b + 1u] = 0u; }
        }
    } else if (lane == 0u) {
        a.status[b] = redo_code;          // decoded again, with the reference's check order, by lz4_decompress_blocks_kernel
        a.out_len[b] = 0u;
    }
}

}  // namespace sq

// Every form of a batch (lz4_device.h): irregular blocks get status `redo_code`; the caller runs launch_decompress with the same
// (d, partial) and only_status = redo_code behind this launch.
template <class SRC, bool PARTIAL>
static hipError_t launch_seq(const DecompressArgs& a, int32_t redo_code, const SRC& src, hipStream_t s) {
    typedef sq::Geo<LZ4S_R, LZ4S_KEEP> G;
    static_assert(G::LDS <= 65536u, "the default limit of dynamic LDS: no function attribute to set per device");
    hipLaunchKernelGGL((sq::lz4_decompress_seq_kernel<G, SRC, PARTIAL>), dim3(a.n), dim3(64), G::LDS, s, a, redo_code, src);
    return hipGetLastError();
}

hipError_t launch_decompress_seq(const DecompressArgs& a, const DictSource& d, bool partial, int32_t redo_code, hipStream_t s) {
    if (a.n == 0u) return hipSuccess;
    if (!decode_form_ok(a, d, partial) || a.dict_base != nullptr || a.chain_done != nullptr) return hipErrorInvalidValue;       // (the plain form: a prefix -- out_pos -- is fine, see the kernel)
    switch ((d.has_set ? 4 : d.shared != nullptr ? 2 : 0) + (partial ? 1 : 0)) {
        case 0: return launch_seq<NoDict, false>(a, redo_code, NoDict{}, s);
        case 1: return launch_seq<NoDict, true>(a, redo_code, NoDict{}, s);
        case 2: return launch_seq<OneDict, false>(a, redo_code, OneDict{d.shared, d.shared_len}, s);
        case 3: return launch_seq<OneDict, true>(a, redo_code, OneDict{d.shared, d.shared_len}, s);
        case 4: return launch_seq<DictSetArgs, false>(a, redo_code, d.set, s);
        default: return launch_seq<DictSetArgs, true>(a, redo_code, d.set, s);
    }
}

}  // namespace lz4flex_dev

#ifdef LZ4S_PROF
extern "C" int lz4flex_debug_seq_prof(unsigned long long* vals, int reset) {
    if (reset) {
        unsigned long long z[32] = {0};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(lz4flex_dev::sq::g_sq_prof), z, sizeof z);
        return 0;
    }
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(vals, HIP_SYMBOL(lz4flex_dev::sq::g_sq_prof), 256);
    return 0;
}
#endif
