// lz4_size_scan.hip -- batched decompressed-size query for raw LZ4 blocks, gfx950 (lz4flex_decompressed_size_batch).
//
// For every block: the number of bytes lz4_flex::block::decompress_into (src/block/decompress.rs:201-449) would produce with an
// unbounded sink and `history` bytes in front of the block's output, or the DecompressError it would return.  Nothing is decoded: only
// the token chain is followed, the lengths summed, and the checks that need a position (offset <= position, :399-401) made.
//
// Two passes, the scheme of the decoders (lz4_decompress_seq.hip + lz4_decompress.hip):
//   * PARALLEL (lz4_size_scan_kernel): one block per WAVEFRONT, the shape of the sequence decoder without its copies and window.  The
//     compressed stream is staged in LDS in tiles of 3 840 bytes (zeros behind the block); 64 lanes walk 64 parts of a tile from
//     assumed entries and the true chain is resolved from the tile's entry (the WALK of lz4_decompress_seq.hip, copied here: that kernel
//     is left as it is), the set bits of the live parts are the tile's token list.  Then CHUNKS of 64 consecutive sequences, lane =
//     sequence: token, literal length, offset and match length from the staged tile, a DPP prefix sum of literal + match lengths places
//     all 64, and every reference check is one ballot (literals past the input :346-348, an offset missing :373-375, offset zero
//     :168-173, offset behind the output :399-401, a match that ends the block :439-443).  A sequence whose lengths do not fit a lane
//     (a literal run of more than LITMAX bytes, any length with a 255 byte) is measured by the whole wavefront from memory, 64 length
//     bytes per load.  A block with anything suspicious -- every error, a position beyond POS_LIMIT, a walk that does not settle -- is
//     marked REDO and left alone.
//   * SERIAL (lz4_size_serial_kernel): one LANE per marked block, the reference's loop restated line by line with 64-bit positions:
//     the error variant comes from code in the reference's check order.  "size_scan_serial" 1 sends every block there (tests).
// LDS per wavefront: token list 2 560 + tile 4 080 = 6 640 bytes.  Nothing is written but out_size[b] and status[b].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4_device.h"
#include "lz4_pcd_common.h"

namespace lz4flex_dev {
namespace ss {

typedef __attribute__((address_space(3))) uint8_t lds_u8;
typedef __attribute__((address_space(3))) uint16_t lds_u16;
typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(1))) uint8_t g_u8;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
using pcd::X_END;
using pcd::X_ERR;

constexpr uint32_t PB = 60u;                 // bytes per part (an odd number of dwords: lane k reading part k hits its own bank)
constexpr uint32_t NPART = 64u;              // parts per tile = lanes
constexpr uint32_t PT = PB * NPART;          // 3 840 compressed bytes per tile
constexpr uint32_t TPAD = 16u;               // bytes in front of the tile
constexpr uint32_t TMARGIN = 224u;           // bytes behind the tile staged with it
constexpr uint32_t TILE_LDS = TPAD + PT + TMARGIN;
constexpr uint32_t POSCAP = PT / 3u;         // sequences per tile: a sequence with a match is at least 3 bytes
constexpr uint32_t POS_LDS = (2u * POSCAP + 15u) & ~15u;
constexpr uint32_t LITMAX = 192u;            // literal run whose offset and match length a lane reads from the staged tile
constexpr uint32_t POS_LIMIT = 0xFFFF0000u;  // output positions of the parallel pass stay below this (beyond: the serial pass, 64-bit)
constexpr uint32_t WALK_LITMAX = 200u;       // literal run a hop steps over without the generic walker
constexpr uint32_t LDS_POS = 0u, LDS_TILE = LDS_POS + POS_LDS;
constexpr uint32_t LDS_BYTES = LDS_TILE + TILE_LDS;
static_assert(TILE_LDS % 16u == 0u && PT % 16u == 0u && POS_LDS % 16u == 0u && PB % 4u == 0u && (PB / 4u) % 2u == 1u && PB <= 64u, "geometry");
static_assert(PT - 1u + 4u + 15u + WALK_LITMAX + 4u < PT + TMARGIN, "a hop's length byte lies inside the staged bytes");
// a token at PT - 1: literals from PT + 1, LITMAX of them, then the offset and a match length byte, read as two aligned dwords
static_assert(((PT + 1u + LITMAX) & ~3u) + 8u <= PT + TMARGIN, "a lane's offset and match length byte lie inside the staged bytes");

#define SS_JOIN() asm volatile("; join")
#define LZ4SS_DPP(v, ctrl, rmask) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), (ctrl), (rmask), 0xf, false))
__device__ __forceinline__ uint32_t wave_incl_add(uint32_t v) {
    v += LZ4SS_DPP(v, 0x111, 0xf);     // row_shr:1
    v += LZ4SS_DPP(v, 0x112, 0xf);     // row_shr:2
    v += LZ4SS_DPP(v, 0x114, 0xf);     // row_shr:4
    v += LZ4SS_DPP(v, 0x118, 0xf);     // row_shr:8
    v += LZ4SS_DPP(v, 0x142, 0xa);     // row_bcast:15 -> rows 1, 3
    v += LZ4SS_DPP(v, 0x143, 0xc);     // row_bcast:31 -> rows 2, 3
    return v;
}
__device__ __forceinline__ uint32_t rdlane(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t ballot(bool b) { return __builtin_amdgcn_ballot_w64(b); }
__device__ __forceinline__ bool lanes(uint64_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
__device__ __forceinline__ uint32_t ctz64(uint64_t x) { return (uint32_t)__builtin_ctzll(x); }
__device__ __forceinline__ uint64_t low_mask(uint32_t n) { return n >= 64u ? ~0ull : (1ull << n) - 1ull; }
__device__ __forceinline__ uint32_t bperm(uint32_t lane_src, uint32_t v) { return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(lane_src * 4u), (int)v); }

__device__ __forceinline__ lds_u8* L8(uint32_t a) { return (lds_u8*)(uintptr_t)a; }
__device__ __forceinline__ void lds_wr16(uint32_t a, const u32x4& v) { __builtin_memcpy((void*)L8(a), &v, 16); }
__device__ __forceinline__ void lds_wr4(uint32_t a, uint32_t v) { __builtin_memcpy((void*)L8(a), &v, 4); }
__device__ __forceinline__ void lds_wr2(uint32_t a, uint32_t v) { const uint16_t t = (uint16_t)v; __builtin_memcpy((void*)L8(a), &t, 2); }
__device__ __forceinline__ uint32_t lds_rd4u(uint32_t a) {
    const lds_u32* q = (const lds_u32*)(uintptr_t)(a & ~3u);
    const uint32_t d0 = q[0], d1 = q[1];
    return __builtin_amdgcn_alignbyte(d1, d0, a & 3u);
}

// ---- the WALK (lz4_decompress_seq.hip, positions only) ---------------------------------------------------------------------------
struct Reader {
    const g_u8* g;
    uint32_t t0;
    __device__ __forceinline__ uint32_t operator()(uint32_t pos) const {
        const uint32_t r = pos - t0;
        return r < PT + TMARGIN ? (uint32_t)*L8(LDS_TILE + TPAD + r) : (uint32_t)g[pos];
    }
    __device__ __forceinline__ uint32_t u32(uint32_t pos) const { return (*this)(pos) | ((*this)(pos + 1u) << 8) | ((*this)(pos + 2u) << 16) | ((*this)(pos + 3u) << 24); }
};
__device__ __noinline__ uint32_t slow_next(const g_u8* g, uint32_t t0, uint32_t ilen, uint32_t p) {
    Reader rd;
    rd.g = g; rd.t0 = t0;
    pcd::Seq q;
    const uint32_t nx = pcd::parse_seq<Reader, false>(rd, ilen, p, q);
    return nx == X_END ? ilen : nx;
}

struct Part {           // positions relative to the tile's first byte t0
    uint64_t marks;      // token positions of the standing walk, relative to the part's first byte
    uint32_t from;       // where the standing walk began (X_ERR: none)
    uint32_t exit;       // where its chain leaves the part, or X_ERR
};

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
        const uint32_t nx = slow_next(g, t0, ilen, t0 + r);
        if (nx == X_ERR) break;
        m2 |= bit;
        r = nx - t0;
    }
    if (merged) { s.marks = m2 | (s.marks & ~((1ull << (r - p0)) - 1ull)); s.from = entry; }
    else { s.marks = m2; s.from = entry; s.exit = exit_; }
}

// ---- measuring --------------------------------------------------------------------------------------------------------------------
// a length run at q (read_integer, decompress.rs:160-174 via :336-340 / :386-391), 64 bytes per load: adds its value to v, q behind it.
// false: the input ends inside the run, or v passes POS_LIMIT
__device__ __forceinline__ bool run_len(const g_u8* in, uint32_t ilen, uint32_t lane, uint32_t& q, uint32_t& v) {
    for (;;) {
        const uint32_t p = q + lane;
        const uint32_t b = p < ilen ? (uint32_t)in[p] : 255u;
        const uint64_t stop = ballot(p < ilen && b != 255u);
        SS_JOIN();
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
// produced in front of it (advanced).  false: an error, or a size beyond POS_LIMIT -- the serial pass names it.  done: the block ended here.
__device__ bool measure_seq(const g_u8* in, uint32_t ilen, uint32_t lane, uint32_t hist, uint32_t ip, uint32_t& op, bool& done) {
    const uint32_t t = uni(in[ip]);
    ip += 1u;
    uint32_t lit = t >> 4;
    if (lit == 15u && !run_len(in, ilen, lane, ip, lit)) return false;
    if (lit > ilen - ip || (uint64_t)op + lit > POS_LIMIT) return false;
    op += lit;
    ip += lit;
    if (ip >= ilen) { done = true; return true; }
    if (ilen - ip < 2u) return false;
    const uint32_t offset = uni((uint32_t)in[ip] | ((uint32_t)in[ip + 1u] << 8));
    ip += 2u;
    if (offset == 0u) return false;
    uint32_t ml = 4u + (t & 15u);
    if (ml == 19u && !run_len(in, ilen, lane, ip, ml)) return false;
    if ((uint64_t)offset > (uint64_t)op + hist) return false;
    if ((uint64_t)op + ml > POS_LIMIT) return false;
    op += ml;
    if (ip >= ilen) return false;              // a match is always followed by another token (:439-443)
    return true;
}

// The sequences [0, n_tile) of the tile's token list, 64 at a time.  op advances; false: the block goes to the serial pass.
__device__ __forceinline__ bool run_chunks(const g_u8* in, uint32_t ilen, uint32_t lane, uint32_t hist, uint32_t t0, uint32_t n_tile,
                                           uint32_t& op, bool& done) {
    const uint32_t ilr = ilen - t0;
    const uint32_t tb = LDS_TILE + TPAD;
    uint32_t sidx = 0u;
    while (sidx < n_tile) {
        sidx = uni(sidx); op = uni(op);
        const uint32_t nrem = n_tile - sidx;
        const uint32_t idx = sidx + (lane < nrem ? lane : nrem - 1u);
        const uint32_t tpr = (uint32_t)*(const lds_u16*)(uintptr_t)(LDS_POS + 2u * idx);
        // token, lengths, offset (decompress.rs:249-258, 334-391)
        const uint32_t w = lds_rd4u(tb + tpr);
        const uint32_t L = (w >> 4) & 15u, M = w & 15u, e1 = (w >> 8) & 0xFFu;
        const bool l15 = L == 15u;
        const uint32_t lit = l15 ? 15u + e1 : L;
        const uint32_t lsr = tpr + (l15 ? 2u : 1u);
        const uint64_t biglit = ballot(lit > LITMAX);           // (covers a length byte of 255)
        const uint32_t lend = lit > LITMAX ? 0u : lsr + lit;
        const uint32_t w1 = lds_rd4u(tb + lend);
        const uint32_t off = w1 & 0xFFFFu, e2 = (w1 >> 16) & 0xFFu;
        const bool m15 = M == 15u;
        const uint32_t mlx = 4u + M + (m15 ? e2 : 0u);
        const uint32_t nxt = lend + (m15 ? 3u : 2u);               // the next token
        const uint64_t lastm = ballot(lend >= ilr);                // the block's last sequence: literals only (:366-368) -- or an error
        const uint64_t errm = ballot(l15 && tpr + 1u >= ilr) | ballot(lend > ilr) |                         // :336-340, :346-348
                              (~lastm & (ballot(lend + 2u > ilr) | ballot(nxt >= ilr) | ballot(off == 0u))); // :373-375, :439-443, :168-173
        const uint64_t bigm = biglit | (~lastm & ballot(m15 && e2 == 255u));                               // more length bytes
        uint32_t nact = nrem < 64u ? nrem : 64u;
        {
            const uint64_t bm = bigm & low_mask(nact);
            if (bm != 0ull) nact = ctz64(bm);
        }
        if (nact == 0u) {                                      // the sequence alone, by the whole wavefront
            const uint32_t tp0 = rdlane(tpr, 0u);
            if (!measure_seq(in, ilen, lane, hist, t0 + tp0, op, done)) return false;
            sidx += 1u;
            if (done) return sidx == n_tile;
            continue;
        }
        const uint64_t am = low_mask(nact);
        if ((errm & am) != 0ull) return false;
        if ((lastm & low_mask(nact - 1u)) != 0ull) return false;   // (a token behind the block's last sequence: not a real chain)
        const uint32_t ml = lanes(lastm) ? 0u : mlx;
        const uint32_t u = lanes(am) ? lit + ml : 0u;
        const uint32_t incl = wave_incl_add(u);
        const uint32_t T = rdlane(incl, nact - 1u);
        if ((uint64_t)op + T > POS_LIMIT) return false;
        const uint32_t dm = op + incl - u + lit;               // output position of the match
        if ((ballot((uint64_t)off > (uint64_t)dm + hist) & ~lastm & am) != 0ull) return false;   // OffsetOutOfBounds (:399-401)
        op += T;
        sidx += nact;
        if (((lastm >> (nact - 1u)) & 1ull) != 0ull) { done = true; return sidx == n_tile; }
    }
    return true;
}

__global__ void __launch_bounds__(64) lz4_size_scan_kernel(const uint8_t* in_base, const uint64_t* in_off, const uint32_t* in_len,
                                                          const uint32_t* history, uint32_t n, uint64_t* out_size, int32_t* status,
                                                          int32_t redo_code) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ss_lds[];
    const uint32_t lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    if (b >= n) return;
    // (every LDS access below goes by byte address from 0: the dynamic segment is the kernel's only LDS)
    if ((uint32_t)(uintptr_t)(lds_u8*)ss_lds != 0u) { if (lane == 0u) { status[b] = redo_code; out_size[b] = 0u; } return; }
    const g_u8* in = (const g_u8*)(in_base + in_off[b]);
    const uint32_t ilen = in_len[b];
    const uint32_t hist = history != nullptr ? uni(history[b]) : 0u;
    bool ok = ilen != 0u && ilen <= POS_LIMIT, done = false;   // (the empty block, decompress.rs:207-209: the serial pass reports it)
    uint32_t op = 0u, entry = 0u;
    if (lane < 4u) lds_wr4(LDS_TILE + 4u * lane, 0u);         // the bytes in front of the first tile
    for (;;) {
        entry = uni(entry); op = uni(op);
        if (uni((ok && !done) ? 1u : 0u) == 0u) break;
        const uint32_t t0 = entry & ~15u;
        // ---- stage the tile: [t0, t0 + PT + TMARGIN), zeros behind the block (reads stay inside [0, ilen)) ----------------------
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
            SS_JOIN();
        }
        // ---- first walks: lane 0 from the tile's entry, the others from their part's first byte --------------------------------------
        const uint32_t ilr = ilen - t0;
        const uint32_t p0 = PB * lane;
        const uint32_t pend = p0 + PB < ilr ? p0 + PB : ilr;
        const uint32_t entry_r = entry - t0;
        Part s;
        s.marks = 0ull; s.from = X_ERR; s.exit = X_ERR;
        if (p0 < ilr) walk_part<true>(in, t0, ilen, lane == 0u ? entry_r : p0, p0, pend, s);
        SS_JOIN();
        // ---- which parts does the true chain visit, and where does it enter them? ------------------------------------------------------
        uint32_t my_entry = X_ERR;
        uint64_t path = 1ull;
        bool settled = false;
        const uint32_t nparts = ilr < PT ? (ilr + PB - 1u) / PB : NPART;
        for (uint32_t round = 0u; round < NPART + 2u; ++round) {
            const bool inside = s.exit != X_ERR && s.exit < PT && s.exit < ilr;
            const uint32_t nxt = inside ? s.exit / PB : 64u;
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
            SS_JOIN();
            path = ((uint64_t)uni((uint32_t)(path >> 32)) << 32) | uni((uint32_t)path);
            if (my_entry != X_ERR && s.from != my_entry && my_entry - p0 < 64u && ((s.marks >> (my_entry - p0)) & 1ull) != 0ull) {
                s.marks &= ~((1ull << (my_entry - p0)) - 1ull);
                s.from = my_entry;
            }
            SS_JOIN();
            const uint64_t needm = ballot(my_entry != X_ERR && s.from != my_entry);
            if (needm == 0ull) { settled = true; break; }
            if (lanes(needm)) walk_part<false>(in, t0, ilen, my_entry, p0, pend, s);
            SS_JOIN();
        }
        settled = uni(settled ? 1u : 0u) != 0u;
        path = ((uint64_t)uni((uint32_t)(path >> 32)) << 32) | uni((uint32_t)path);
        const uint32_t tile_exit = settled ? rdlane(s.exit, 63u - (uint32_t)__builtin_clzll(path)) : X_ERR;
        if (tile_exit == X_ERR) { ok = false; break; }
        // ---- the token list ----------------------------------------------------------------------------------------------------------
        uint64_t m = my_entry != X_ERR ? s.marks : 0ull;
        const uint32_t cnt = (uint32_t)__builtin_popcountll(m);
        const uint32_t cincl = wave_incl_add(cnt);
        const uint32_t n_tile = rdlane(cincl, 63u);
        if (n_tile > POSCAP || n_tile == 0u) { ok = false; break; }
        {
            uint32_t at = LDS_POS + 2u * (cincl - cnt);
            while (ballot(m != 0ull) != 0ull) {
                if (m != 0ull) {
                    lds_wr2(at, p0 + ctz64(m));
                    at += 2u;
                    m &= m - 1ull;
                }
                SS_JOIN();
            }
        }
        // ---- the sequences -----------------------------------------------------------------------------------------------------------
        bool tdone = false;
        if (!run_chunks(in, ilen, lane, hist, t0, n_tile, op, tdone)) { ok = false; break; }
        if (tdone) { done = true; break; }
        if (tile_exit >= ilr) { ok = false; break; }        // the chain ran out without a last sequence
        entry = t0 + tile_exit;
    }
    if (lane == 0u) {
        if (ok && done) { status[b] = 0; out_size[b] = op; }
        else { status[b] = redo_code; out_size[b] = 0u; }
    }
}

// ---- the serial pass: decompress.rs:201-449 for one block per lane, lengths only, 64-bit positions -----------------------------------
__device__ __forceinline__ int32_t read_integer(const uint8_t* in, uint64_t ilen, uint64_t& ip, uint64_t& v) {   // :160-174
    for (;;) {
        if (ip >= ilen) return LZ4FLEX_DEV_E_EXPECTED_ANOTHER_BYTE;
        const uint32_t extra = in[ip++];
        v += extra;
        if (extra != 0xFFu) return 0;
    }
}
__device__ int32_t measure_block(const uint8_t* in, uint64_t ilen, uint64_t hist, uint64_t& size) {
    if (ilen == 0u) return LZ4FLEX_DEV_E_EXPECTED_ANOTHER_BYTE;           // :207-209
    uint64_t ip = 0u, op = 0u;
    for (;;) {
        const uint32_t token = in[ip++];                                  // :249-250
        uint64_t lit = token >> 4;                                        // :334
        if (lit != 0u) {
            if (lit == 15u) {                                             // :336-340
                const int32_t e = read_integer(in, ilen, ip, lit);
                if (e) return e;
            }
            if (lit > ilen - ip) return LZ4FLEX_DEV_E_LITERAL_OUT_OF_BOUNDS;      // :346-348
            op += lit;
            ip += lit;
        }
        if (ip >= ilen) break;                                            // :366-368
        if (ilen - ip < 2u) return LZ4FLEX_DEV_E_EXPECTED_ANOTHER_BYTE;  // :373-375
        const uint64_t offset = (uint64_t)in[ip] | ((uint64_t)in[ip + 1u] << 8);
        ip += 2u;
        if (offset == 0u) return LZ4FLEX_DEV_E_OFFSET_ZERO;               // :168-173
        uint64_t ml = 4u + (token & 0xFu);                                // :386-391
        if (ml == 19u) {
            const int32_t e = read_integer(in, ilen, ip, ml);
            if (e) return e;
        }
        if (offset > op + hist) return LZ4FLEX_DEV_E_OFFSET_OUT_OF_BOUNDS;        // :399-401
        op += ml;
        if (ip >= ilen) return LZ4FLEX_DEV_E_EXPECTED_ANOTHER_BYTE;       // :439-443
    }
    size = op;
    return 0;
}

__global__ void __launch_bounds__(256) lz4_size_serial_kernel(const uint8_t* in_base, const uint64_t* in_off, const uint32_t* in_len,
                                                             const uint32_t* history, uint32_t n, uint64_t* out_size, int32_t* status,
                                                             int32_t only_status) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= n) return;
    if (only_status != 0 && status[b] != only_status) return;
    uint64_t size = 0u;
    const int32_t st = measure_block(in_base + in_off[b], in_len[b], history != nullptr ? history[b] : 0u, size);
    status[b] = st;
    out_size[b] = st == 0 ? size : 0u;
}

}  // namespace ss

hipError_t launch_size_scan(const uint8_t* in_base, const uint64_t* in_off, const uint32_t* in_len, const uint32_t* history, uint32_t n,
                            uint64_t* out_size, int32_t* status, int serial_only, hipStream_t s) {
    if (n == 0u) return hipSuccess;
    const int32_t redo = SIZE_SCAN_REDO;
    if (!serial_only) {
        hipLaunchKernelGGL(ss::lz4_size_scan_kernel, dim3(n), dim3(64), ss::LDS_BYTES, s, in_base, in_off, in_len, history, n, out_size,
                           status, redo);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(ss::lz4_size_serial_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, in_base, in_off, in_len, history, n, out_size,
                       status, serial_only ? 0 : redo);
    return hipGetLastError();
}

}  // namespace lz4flex_dev
