// lz4_fit.hip -- a finished LZ4 block cut to a capacity, gfx950 (lz4flex_fit_batch, lz4flex_compress_batch_fit): liblz4's
// LZ4_compress_destSize as a pass over the block, the mirror image of the partial decode.
//
// For every block B (which decodes to the n = src_len bytes of its source) and capacity cap: B itself when it fits, else the best cut --
// the sequences in front of a sequence k unchanged, then either a final run of literals (Plain(k)) or sequence k with its match
// shortened and a final run behind it (Clipped(k)), the literals of the final run read from the source.  The RULE -- which k, which
// form, how long -- is stated in include/lz4flex_amd.h and, as a program, in tests/fit_model.py; best_of_seq below is that rule for one k.
//
// Two passes, the scheme of the size scan (lz4_size_scan.hip):
//   * PARALLEL (lz4_fit_kernel): one block per WAVEFRONT on the size scan's geometry.  The walk (lz4_seq_walk.h) gives a tile's token
//     list; then CHUNKS of 64 consecutive sequences, lane = sequence: a DPP prefix sum of literal + match lengths is p_k, the token's
//     position c_k, the match in front of it comes by a DPP shift, and every lane evaluates its Plain and its Clipped candidate in
//     closed form.  The chunk's best is a wave maximum over `used`, one over `cap - size` among the lanes that hold it, and the lowest
//     such lane (three steps instead of one 64-bit key: used and cap - size are 32 bits each); the running best lives in SGPRs across
//     chunks and tiles and is replaced only by a strictly better one, so the smallest k wins a tie.  Only sequences whose token lies in
//     front of cap are looked at, and the walk ends with the first tile entered at or behind cap.  A sequence no lane can take (a
//     literal run of more than LITMAX bytes, a length with a 255 byte) is parsed by the whole wavefront and is a candidate like the
//     others -- a 4 MiB run of zeros is one such sequence, and its Clipped cut is what a zero page fits by.  Then the copies, 64 lanes,
//     16 bytes per lane where source and destination allow (lz4_copy_range.h): B[0, c_k), sequence k's head, the final literals.
//     Every error in front of the cut, a position beyond POS_LIMIT, a walk that does not settle: the block is marked REDO, untouched.
//   * SERIAL (lz4_fit_serial_kernel): one LANE per marked block, the rule restated sequence by sequence in the reference's check order
//     (decompress.rs:249-443) with 64-bit positions; an error gives its DecompressError code, out_len 0, in_used 0 and writes
//     nothing.  "fit_serial" 1 sends every block there (tests, A/B); the hook "debug_fit_first_pass" leaves the marked blocks marked.
// Errors behind the cut are not seen (the partial decoder's contract): nothing of a sequence whose token lies at or behind cap is parsed.
// LDS per wavefront: token list 2 560 + tile 4 080 = 6 640 bytes.  No scratch memory; lz4_fit_kernel: 116 VGPRs, lz4_fit_serial_kernel: 68.
// Writes: out[out_off, out_off + out_len) of a block with status 0, out_len, in_used, status; nothing else.  Reads: B below in_len, the
// source below src_len.  Every store is a plain vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4_copy_range.h"
#include "lz4_device.h"
#include "lz4_seq_walk.h"

namespace lz4flex_dev {
namespace fit {

using namespace sw;      // the walk, its geometry and the lane / LDS helpers

constexpr uint32_t LITMAX = 192u;            // literal run whose offset and match length a lane reads from the staged tile
constexpr uint32_t LDS_BYTES = LDS_TILE + TILE_LDS;
static_assert(((PT + 1u + LITMAX) & ~3u) + 8u <= PT + TMARGIN, "a lane's offset and match length byte lie inside the staged bytes");

// ---- the rule for one sequence (T: uint32_t in a lane -- l <= LITMAX, m <= 273, positions below POS_LIMIT --, else uint64_t) -----------
template <typename T> __device__ __forceinline__ T ext_of(T x) { return x < 15u ? (T)0u : (T)(1u + (x - 15u) / 255u); }
template <typename T> __device__ __forceinline__ T tail_of(T L) { return (T)(1u + ext_of<T>(L) + L); }
// the largest L in [0, avail] with tail(L) <= r (r >= 1): L = 15 + x with x + x / 255 <= r - 17 beyond 14
template <typename T> __device__ __forceinline__ T lfit(T r, T avail) {
    T L;
    if (r <= 16u) L = r - 1u < 14u ? r - 1u : (T)14u;
    else { const T y = r - 17u; L = (T)(15u + y - (y >> 8) - ((y & 255u) == 255u ? 1u : 0u)); }
    return L < avail ? L : avail;
}
template <typename T> struct Cand {
    T used, slack, mc, L;      // source bytes the cut block decodes to; cap - its size; Clipped: the match length left; the final run
    uint32_t plain;            // 1 = Plain(k), 0 = Clipped(k)
    bool ok;
};
// the better of Plain(k) and Clipped(k) for the sequence at c < cap that starts at decoded position p: l literals, a match of m bytes
// (0: the block's last sequence); lmin: the shortest final run the end rules allow behind the sequence in front of it
template <typename T> __device__ __forceinline__ Cand<T> best_of_seq(T c, T p, T l, T m, T lmin, T cap, T n) {
    Cand<T> r;
    r.ok = false; r.used = 0u; r.slack = 0u; r.mc = 0u; r.L = 0u; r.plain = 1u;
    const T room = cap - c;
    if (p <= n) {
        const T L = lfit<T>(room, n - p);
        if (L >= lmin) { r.ok = true; r.used = p + L; r.slack = room - tail_of<T>(L); r.L = L; }
    }
    if (m >= 5u && l < room) {
        const T h = (T)(3u + ext_of<T>(l) + l);
        if (room >= h && room - h >= 6u) {
            const T b = room - h - 1u;
            const T steps = b - 5u;
            T mc = m - 1u;
            if (steps <= m / 255u) { const T reach = (T)(18u + 255u * steps); mc = mc < reach ? mc : reach; }
            const T lm = mc >= 7u ? (T)5u : (T)(12u - mc);
            if (lm <= b && p + l + mc <= n) {
                const T r2 = room - h - ext_of<T>(mc - 4u);
                const T L = lfit<T>(r2, n - p - l - mc);
                const T used = p + l + mc + L, slack = r2 - tail_of<T>(L);
                if (L >= lm && (!r.ok || used > r.used || (used == r.used && slack > r.slack))) {
                    r.ok = true; r.used = used; r.slack = slack; r.mc = mc; r.L = L; r.plain = 0u;
                }
            }
        }
    }
    return r;
}

// ---- the running best, wave-uniform ------------------------------------------------------------------------------------------------
struct Best {
    uint32_t have, used, slack, plain, mc, L, c, l;     // c, l: sequence k's token position and literal length
};
__device__ __forceinline__ bool better(const Best& b, uint32_t used, uint32_t slack) {
    return b.have == 0u || used > b.used || (used == b.used && slack > b.slack);
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    v = max(v, LZ4_DPP(v, 0x111, 0xf));     // row_shr:1
    v = max(v, LZ4_DPP(v, 0x112, 0xf));     // row_shr:2
    v = max(v, LZ4_DPP(v, 0x114, 0xf));     // row_shr:4
    v = max(v, LZ4_DPP(v, 0x118, 0xf));     // row_shr:8
    v = max(v, LZ4_DPP(v, 0x142, 0xa));     // row_bcast:15 -> rows 1, 3
    v = max(v, LZ4_DPP(v, 0x143, 0xc));     // row_bcast:31 -> rows 2, 3
    return rdlane(v, 63u);
}

enum : uint32_t { TILE_MORE = 0u, TILE_END = 1u, TILE_REDO = 2u };

// The sequences [0, n_tile) of the tile's token list whose token lies in front of cap, 64 at a time.  op advances, best follows;
// mprev: the match in front of the next sequence (0: the block's first).  TILE_END: the cut lies in this tile or the block ended.
__device__ __forceinline__ uint32_t run_chunks(const g_u8* in, uint32_t ilen, uint32_t lane, uint32_t t0, uint32_t n_tile, uint32_t cap,
                                               uint32_t n, uint32_t& op, uint32_t& mprev, Best& best) {
    const uint32_t ilr = ilen - t0;
    const uint32_t capr = cap - t0;                            // (the tile was entered in front of cap)
    uint32_t sidx = 0u;
    while (sidx < n_tile) {
        sidx = uni(sidx); op = uni(op); mprev = uni(mprev);
        const uint32_t nrem = n_tile - sidx;
        // token, lengths, offset (decompress.rs:249-258, 334-391)
        const Token t = decode_token<LITMAX>(sidx + (lane < nrem ? lane : nrem - 1u), ilr);
        const uint32_t tpr = t.tpr, lit = t.lit, off = t.off, mlx = t.mlx;
        const uint64_t lastm = t.lastm;
        uint64_t errm, bigm;
        chunk_masks(t, ilr, errm, bigm);
        const uint64_t behind = ballot(tpr >= capr);           // tokens at or behind cap: not looked at
        uint32_t nact = nrem < 64u ? nrem : 64u;
        bool cut_here = false;
        {
            const uint64_t bh = behind & low_mask(nact);
            if (bh != 0ull) { nact = ctz64(bh); cut_here = true; }
            const uint64_t bm = bigm & low_mask(nact);
            if (bm != 0ull) { nact = ctz64(bm); cut_here = false; }
        }
        if (nact == 0u) {
            if (cut_here) return TILE_END;
            // the sequence alone, by the whole wavefront
            const uint32_t c = t0 + rdlane(tpr, 0u), p = op;
            uint32_t sl = 0u, sm = 0u;
            bool last = false;
            if (!wave_seq(in, ilen, lane, 0u, c, op, sl, sm, last)) return TILE_REDO;
            const uint64_t lmin = mprev == 0u ? 0u : (mprev >= 7u ? 5u : 12u - mprev);
            const Cand<uint64_t> cd = best_of_seq<uint64_t>(c, p, sl, sm, lmin, cap, n);
            if (cd.ok && better(best, (uint32_t)cd.used, (uint32_t)cd.slack)) {
                best.have = 1u; best.used = (uint32_t)cd.used; best.slack = (uint32_t)cd.slack; best.plain = cd.plain;
                best.mc = (uint32_t)cd.mc; best.L = (uint32_t)cd.L; best.c = c; best.l = sl;
            }
            mprev = sm;
            sidx += 1u;
            if (last) return sidx == n_tile ? TILE_END : TILE_REDO;
            continue;
        }
        const uint64_t am = low_mask(nact);
        if ((errm & am) != 0ull) return TILE_REDO;
        if ((lastm & low_mask(nact - 1u)) != 0ull) return TILE_REDO;   // (a token behind the block's last sequence: not a real chain)
        const bool active = lanes(am);
        const uint32_t ml = lanes(lastm) ? 0u : mlx;
        const uint32_t u = active ? lit + ml : 0u;
        const uint32_t incl = wave_incl_add(u);
        const uint32_t T = rdlane(incl, nact - 1u);
        if ((uint64_t)op + T > POS_LIMIT) return TILE_REDO;
        const uint32_t p = op + incl - u;
        if ((ballot(off > p + lit) & ~lastm & am) != 0ull) return TILE_REDO;     // OffsetOutOfBounds (:399-401)
        // the match in front of this lane's sequence, the end rules' shortest final run behind it
        const uint32_t left = LZ4_DPP(ml, 0x138, 0xf);                         // wave_shr:1
        const uint32_t mp = lane == 0u ? mprev : left;
        const uint32_t lmin = mp == 0u ? 0u : (mp >= 7u ? 5u : 12u - mp);
        const Cand<uint32_t> cd = best_of_seq<uint32_t>(t0 + tpr, p, lit, ml, lmin, cap, n);
        const bool ok = active && cd.ok;
        const uint64_t okm = ballot(ok);
        if (okm != 0ull) {
            const uint32_t mx = wave_max(ok ? cd.used : 0u);
            const uint64_t m1 = ballot(ok && cd.used == mx);
            const uint32_t sx = wave_max(lanes(m1) ? cd.slack : 0u);
            const uint64_t m2 = m1 & ballot(cd.slack == sx);
            if (better(best, mx, sx)) {
                const uint32_t w = ctz64(m2);
                best.have = 1u; best.used = mx; best.slack = sx; best.plain = rdlane(cd.plain, w); best.mc = rdlane(cd.mc, w);
                best.L = rdlane(cd.L, w); best.c = t0 + rdlane(tpr, w); best.l = rdlane(lit, w);
            }
        }
        op += T;
        mprev = rdlane(ml, nact - 1u);
        sidx += nact;
        if (((lastm >> (nact - 1u)) & 1ull) != 0ull) return sidx == n_tile ? TILE_END : TILE_REDO;
        if (cut_here) return TILE_END;
    }
    return TILE_MORE;
}

// v as the length bytes behind a 15-nibble (v = length - 15) at q: floor(v / 255) bytes of 255, then v % 255.  Returns their number.
__device__ __forceinline__ uint32_t put_length(uint8_t* q, uint32_t v, uint32_t lane) {
    const uint32_t full = v / 255u;
    for (uint32_t i = lane; i < full; i += 64u) q[i] = 255u;
    if (lane == 0u) q[full] = (uint8_t)(v - 255u * full);
    return full + 1u;
}

__global__ void __launch_bounds__(64) lz4_fit_kernel(const uint8_t* blk_base, const uint64_t* blk_off, const uint32_t* blk_len,
                                                    const uint8_t* src_base, const uint64_t* src_off, const uint32_t* src_len, uint32_t n_blocks,
                                                    uint8_t* out_base, const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len,
                                                    uint32_t* in_used, int32_t* status, int32_t gated, int32_t redo_code) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fit_lds[];
    const uint32_t lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    if (b >= n_blocks) return;
    if (gated != 0 && status[b] != 0) {                       // (the encoder in front of this pass failed the block: its status stands)
        if (lane == 0u) { out_len[b] = 0u; in_used[b] = 0u; }
        return;
    }
    const uint8_t* blk = blk_base + blk_off[b];
    const uint32_t ilen = uni(blk_len[b]), cap = uni(out_cap[b]), n = uni(src_len[b]);
    uint8_t* out = out_base + out_off[b];
    if (ilen <= cap) {                                         // B fits: the copy alone
        copy_range(out, blk, ilen, lane, 64u);
        if (lane == 0u) { out_len[b] = ilen; in_used[b] = n; status[b] = 0; }
        return;
    }
    if (cap == 0u) {
        if (lane == 0u) { out_len[b] = 0u; in_used[b] = 0u; status[b] = LZ4FLEX_DEV_E_OUTPUT_TOO_SMALL; }
        return;
    }
    // (every LDS access below goes by byte address from 0: the dynamic segment is the kernel's only LDS)
    bool ok = (uint32_t)(uintptr_t)(lds_u8*)fit_lds == 0u && ilen <= POS_LIMIT;
    const g_u8* in = (const g_u8*)blk;
    Best best;
    best.have = 0u; best.used = 0u; best.slack = 0u; best.plain = 1u; best.mc = 0u; best.L = 0u; best.c = 0u; best.l = 0u;
    uint32_t op = 0u, entry = 0u, mprev = 0u;
    if (ok && lane < 4u) lds_wr4(LDS_TILE + 4u * lane, 0u);   // the bytes in front of the first tile
    SW_JOIN();
    for (;;) {
        entry = uni(entry); op = uni(op);
        if (uni(ok ? 1u : 0u) == 0u) break;
        const uint32_t t0 = entry & ~15u;
        stage_tile(in, ilen, t0, lane);
        const uint32_t ilr = ilen - t0;
        const uint32_t entry_r = entry - t0;
        Part s;
        first_walks(in, ilen, t0, lane, entry_r, s);
        uint32_t my_entry, rounds;
        const uint32_t tile_exit = settle_chain(in, ilen, t0, lane, entry_r, s, my_entry, rounds);
        if (tile_exit == X_ERR) { ok = false; break; }
        const uint32_t n_tile = write_token_list(lane, my_entry, s);
        if (n_tile > POSCAP || n_tile == 0u) { ok = false; break; }
        const uint32_t r = run_chunks(in, ilen, lane, t0, n_tile, cap, n, op, mprev, best);
        if (r == TILE_REDO) { ok = false; break; }
        if (r == TILE_END) break;
        if (tile_exit >= ilr) { ok = false; break; }        // the chain ran out without a last sequence
        entry = t0 + tile_exit;
        if (entry >= cap) break;                               // the next token lies at or behind cap
    }
    // ---- the cut block -------------------------------------------------------------------------------------------------------------
    const uint32_t c = uni(best.c), l = uni(best.l), mc = uni(best.mc), L = uni(best.L), used = uni(best.used);
    const bool clipped = uni(best.plain) == 0u;
    const uint64_t h = 3ull + ext_of<uint64_t>(l) + l;         // sequence k up to its offset
    const uint64_t size = (uint64_t)c + (clipped ? h + ext_of<uint64_t>(mc - 4u) : 0ull) + tail_of<uint64_t>(L);
    if (!ok || uni(best.have) == 0u || size > cap || used > n || L > used || (clipped && c + h > ilen)) {    // (the last four: never, by the rule)
        if (lane == 0u) { status[b] = redo_code; out_len[b] = 0u; in_used[b] = 0u; }
        return;
    }
    copy_range(out, blk, c, lane, 64u);
    uint32_t pos = c;
    if (clipped) {
        const uint32_t code = mc - 4u;
        if (lane == 0u) out[pos] = (uint8_t)((blk[pos] & 0xF0u) | (code < 15u ? code : 15u));
        copy_range(out + pos + 1u, blk + pos + 1u, h - 1u, lane, 64u);
        pos += (uint32_t)h;
        if (code >= 15u) pos += put_length(out + pos, code - 15u, lane);
    }
    if (lane == 0u) out[pos] = (uint8_t)((L < 15u ? L : 15u) << 4);
    pos += 1u;
    if (L >= 15u) pos += put_length(out + pos, L - 15u, lane);
    copy_range(out + pos, src_base + src_off[b] + (used - L), L, lane, 64u);
    if (lane == 0u) { out_len[b] = pos + L; in_used[b] = used; status[b] = 0; }
}

// ---- the serial pass: the rule for one block per lane, decompress.rs:249-443's checks for every sequence in front of cap ----------------
__device__ __forceinline__ uint64_t put_length_serial(uint8_t* q, uint64_t v) {
    uint64_t i = 0u;
    for (; v >= 255u; v -= 255u) q[i++] = 255u;
    q[i++] = (uint8_t)v;
    return i;
}
__device__ int32_t fit_block(const uint8_t* B, uint64_t ilen, const uint8_t* src, uint64_t n, uint64_t cap, uint8_t* out, uint32_t& out_len,
                             uint32_t& used) {
    if (ilen <= cap) {
        for (uint64_t i = 0u; i < ilen; ++i) out[i] = B[i];
        out_len = (uint32_t)ilen; used = (uint32_t)n;
        return 0;
    }
    if (cap == 0u) return LZ4FLEX_DEV_E_OUTPUT_TOO_SMALL;
    Cand<uint64_t> best;
    best.ok = false; best.used = 0u; best.slack = 0u; best.mc = 0u; best.L = 0u; best.plain = 1u;
    uint64_t ip = 0u, op = 0u, mprev = 0u, bc = 0u, bl = 0u;
    while (ip < cap) {                                                    // (cap < ilen: there is a token)
        const uint64_t c = ip, p = op;
        const uint32_t token = B[ip++];                                   // :249-250
        uint64_t lit = token >> 4, ml = 0u;                               // :334
        if (lit == 15u) {                                                 // :336-340
            const int32_t e = read_integer(B, ilen, ip, lit);
            if (e) return e;
        }
        if (lit > ilen - ip) return LZ4FLEX_DEV_E_LITERAL_OUT_OF_BOUNDS;          // :346-348
        op += lit;
        ip += lit;
        const bool last = ip >= ilen;                                     // :366-368
        if (!last) {
            if (ilen - ip < 2u) return LZ4FLEX_DEV_E_EXPECTED_ANOTHER_BYTE;      // :373-375
            const uint64_t offset = (uint64_t)B[ip] | ((uint64_t)B[ip + 1u] << 8);
            ip += 2u;
            if (offset == 0u) return LZ4FLEX_DEV_E_OFFSET_ZERO;           // :168-173
            ml = 4u + (token & 0xFu);                                     // :386-391
            if (ml == 19u) {
                const int32_t e = read_integer(B, ilen, ip, ml);
                if (e) return e;
            }
            if (offset > op) return LZ4FLEX_DEV_E_OFFSET_OUT_OF_BOUNDS;   // :399-401
            op += ml;
            if (ip >= ilen) return LZ4FLEX_DEV_E_EXPECTED_ANOTHER_BYTE;   // :439-443
        }
        const uint64_t lmin = mprev == 0u ? 0u : (mprev >= 7u ? 5u : 12u - mprev);
        const Cand<uint64_t> cd = best_of_seq<uint64_t>(c, p, lit, ml, lmin, cap, n);
        if (cd.ok && (!best.ok || cd.used > best.used || (cd.used == best.used && cd.slack > best.slack))) { best = cd; bc = c; bl = lit; }
        if (last) break;
        mprev = ml;
    }
    if (!best.ok) return LZ4FLEX_DEV_E_OUTPUT_TOO_SMALL;                  // (never: Plain(0) is legal at every cap >= 1)
    for (uint64_t i = 0u; i < bc; ++i) out[i] = B[i];
    uint64_t pos = bc;
    if (best.plain == 0u) {
        const uint64_t h = 3u + ext_of<uint64_t>(bl) + bl, code = best.mc - 4u;
        out[pos] = (uint8_t)((B[pos] & 0xF0u) | (code < 15u ? code : 15u));
        for (uint64_t i = 1u; i < h; ++i) out[pos + i] = B[pos + i];
        pos += h;
        if (code >= 15u) pos += put_length_serial(out + pos, code - 15u);
    }
    out[pos++] = (uint8_t)((best.L < 15u ? best.L : 15u) << 4);
    if (best.L >= 15u) pos += put_length_serial(out + pos, best.L - 15u);
    const uint8_t* lits = src + (best.used - best.L);
    for (uint64_t i = 0u; i < best.L; ++i) out[pos + i] = lits[i];
    out_len = (uint32_t)(pos + best.L); used = (uint32_t)best.used;
    return 0;
}

__global__ void __launch_bounds__(256) lz4_fit_serial_kernel(const uint8_t* blk_base, const uint64_t* blk_off, const uint32_t* blk_len,
                                                            const uint8_t* src_base, const uint64_t* src_off, const uint32_t* src_len,
                                                            uint32_t n_blocks, uint8_t* out_base, const uint64_t* out_off, const uint32_t* out_cap,
                                                            uint32_t* out_len, uint32_t* in_used, int32_t* status, int32_t gated, int32_t only_status) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= n_blocks) return;
    if (only_status != 0) { if (status[b] != only_status) return; }
    else if (gated != 0 && status[b] != 0) { out_len[b] = 0u; in_used[b] = 0u; return; }
    uint32_t len = 0u, used = 0u;
    const int32_t st = fit_block(blk_base + blk_off[b], blk_len[b], src_base + src_off[b], src_len[b], out_cap[b], out_base + out_off[b], len, used);
    status[b] = st;
    out_len[b] = st == 0 ? len : 0u;
    in_used[b] = st == 0 ? used : 0u;
}

}  // namespace fit

hipError_t launch_fit(const FitArgs& a, int gated, int serial_only, hipStream_t s) {
    if (a.n == 0u) return hipSuccess;
    const int32_t redo = FIT_REDO;
    if (serial_only != 1) {
        hipLaunchKernelGGL(fit::lz4_fit_kernel, dim3(a.n), dim3(64), fit::LDS_BYTES, s, a.blk_base, a.blk_off, a.blk_len, a.src_base, a.src_off,
                           a.src_len, a.n, a.out_base, a.out_off, a.out_cap, a.out_len, a.in_used, a.status, (int32_t)gated, redo);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess || serial_only == 2) return e;
    }
    hipLaunchKernelGGL(fit::lz4_fit_serial_kernel, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a.blk_base, a.blk_off, a.blk_len, a.src_base,
                       a.src_off, a.src_len, a.n, a.out_base, a.out_off, a.out_cap, a.out_len, a.in_used, a.status, (int32_t)gated,
                       serial_only == 1 ? 0 : redo);
    return hipGetLastError();
}

}  // namespace lz4flex_dev
