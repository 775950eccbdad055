// lz4_compress_high.hip -- compress_mode 2 ("high"): a deep-search encoder for independent blocks, without a dictionary (the plain form)
// and against one ("compress_high_dict" 1: the dictionary form, the same code as a template on the dictionary; "compress_high_linked" 1:
// the same form with the block's own stream as its dictionary, LZ4FLEX_BLOCK_HISTORY).
//
// The bytes are DEFINED by the scalar model tests/sim/high_encoder_model.c (chunks, candidates, best[], the one-step lazy parse: see its
// head comment and include/lz4flex_amd.h, "compress_mode"); this kernel computes the same function of (block, depth) in parallel.  The
// dictionary form's definition is tests/sim/high_dict_model.c: the dictionary's last H <= 32 KiB bytes are chunk 0's history, every chunk
// is 32 KiB, and nothing else changes -- here the differences are confined to chunk 0 (its geometry, stage_dict, the sort's enumeration
// and, with the shared dictionary's digest, where a position's candidates come from).
//
// Persistent workgroups of 1 024 lanes; workgroup w takes the blocks w, w + G, w + 2 G, ... and a block's chunks one after the other.  No
// workgroup ever waits for another one.  Per chunk (a window of at most 64 KiB: 32 KiB of history + the chunk; chunk 0: the chunk alone):
//   1  stage     the window into LDS as aligned dwords (every later read of it is a dword pair / triple and a shift)
//   2  sort      the window's positions, stably, by their 15-bit hash: three counting passes of 5 bits, 512 segments with private
//                counter columns in LDS, the arrays in the workgroup's slice of the workspace (L2).  Behind it the candidates of a position
//                are its LEFT NEIGHBOURS in the sorted array, nearest first -- no chains to chase.
//   3  match     a lane per sorted index: up to `depth` left neighbours, 8 bytes per compare step; best[] (length, offset) to the workspace
//   3 1/2        ("compress_parse" 1 only: tests/sim/high_optimal_model.c) best[].len becomes len'[], the length the optimal parse takes at
//                each position -- a backward pass over prices, a wavefront per segment of 2 048 positions (optimal_lengths)
//   4  orbit     the parse is the orbit of the chunk's first position under next(p) (p + 1 for a literal, p + len for a match): a lane
//                per tile of 64 positions computes every entry's exit (backwards, one pass), one lane hops from tile to tile, then a
//                lane per entered tile counts and lists its matches (the window's LDS is free by then)
//   5  sizes     a lane per sequence, a prefix sum
//   6  emit      a lane per sequence; literal runs of 1 KiB or more are copied by the whole workgroup
// Every step but 3 1/2 is a loop over items strided by the lanes, between workgroup barriers, without wavefront-level operations.
#include "lz4_device.h"
#include <algorithm>

namespace lz4flex_dev {
namespace high {

constexpr uint32_t THREADS = 1024u;
constexpr uint32_t CHUNK0 = 65536u, CHUNK = 32768u;      // the model's LZ4H_CHUNK0 / LZ4H_CHUNK
constexpr uint32_t HASH_BITS = 15u;
constexpr uint32_t SEGS = 512u, DIGIT_BITS = 5u, DIGITS = 1u << DIGIT_BITS;      // the sort: 3 passes of 5 bits
constexpr uint32_t TILE = 64u;
constexpr uint32_t MAX_SEQS = CHUNK0 / 4u;               // a match is 4 bytes or more
constexpr uint32_t LONG_LIT = 1024u, MAX_LONG = CHUNK0 / LONG_LIT + 1u;
constexpr uint32_t NONE = 0xFFFFFFFFu;

// LDS.  [0, L_BIG_END) is, one after the other: the window + the sort's counters | the exits (u16 per position) | the sequence lists
constexpr uint32_t WIN_BYTES = CHUNK0 + 32u;             // the window from the aligned dword in front of it, and a triple's slack
constexpr uint32_t L_CNT = WIN_BYTES;                    // u32[DIGITS * SEGS]
constexpr uint32_t L_BIG_END = L_CNT + 4u * DIGITS * SEGS;
constexpr uint32_t L_SEQPOS = 0u, L_SEQOFF = 4u * MAX_SEQS;
constexpr uint32_t L_ENTRY = L_BIG_END;                  // u32[CHUNK0 / TILE]: where the orbit enters a tile
constexpr uint32_t L_TCNT = L_ENTRY + 4u * (CHUNK0 / TILE);
constexpr uint32_t L_TMP = L_TCNT + 4u * (CHUNK0 / TILE);      // u32[THREADS]: block_scan
constexpr uint32_t L_MISC = L_TMP + 4u * THREADS;        // [0] the number of long literal runs, [1 ..] their sequences
constexpr uint32_t LDS_BYTES = L_MISC + 4u * (1u + MAX_LONG + 2u);
static_assert(2u * CHUNK0 <= L_BIG_END && 8u * MAX_SEQS <= L_BIG_END, "the exits and the sequence lists reuse the window's LDS");
static_assert(LDS_BYTES <= 160u * 1024u, "one workgroup per CU");

// the workgroup's slice of the workspace
constexpr size_t W_SORT_A = 0, W_SORT_B = 2u * CHUNK0, W_LEN = 4u * CHUNK0, W_OFF = W_LEN + 2u * (CHUNK0 + 64u);
constexpr size_t WS_PER_WG = (W_OFF + 2u * CHUNK0 + 255u) & ~(size_t)255u;

__device__ __forceinline__ uint32_t umin(uint32_t x, uint32_t y) { return x < y ? x : y; }
__device__ __forceinline__ uint32_t hash_of(uint32_t v) { return (v * 2654435761u) >> (32u - HASH_BITS); }
// 4 / 8 / 1 bytes at byte offset x of the dword array w (LDS)
__device__ __forceinline__ uint32_t ld32(const uint32_t* w, uint32_t x) {
    const uint32_t i = x >> 2;
    return (uint32_t)((((uint64_t)w[i + 1u] << 32) | w[i]) >> ((x & 3u) * 8u));
}
__device__ __forceinline__ uint64_t ld64(const uint32_t* w, uint32_t x) {
    const uint32_t i = x >> 2, sh = (x & 3u) * 8u;
    const uint64_t lo = ((uint64_t)w[i + 1u] << 32) | w[i];
    return sh ? (lo >> sh) | ((uint64_t)w[i + 2u] << (64u - sh)) : lo;
}
__device__ __forceinline__ uint32_t ld8(const uint32_t* w, uint32_t x) { return (w[x >> 2] >> ((x & 3u) * 8u)) & 255u; }
// the length bytes behind a token nibble of 15
__device__ __forceinline__ uint32_t ext_bytes(uint32_t v) { return v >= 15u ? (v - 15u) / 255u + 1u : 0u; }
__device__ __forceinline__ uint8_t* put_ext(uint8_t* o, uint32_t v) {
    if (v >= 15u) {
        v -= 15u;
        for (; v >= 255u; v -= 255u) *o++ = 255u;
        *o++ = (uint8_t)v;
    }
    return o;
}

// a[0, n) becomes its exclusive prefix sums, in place; returns the total.  tmp: blockDim.x words.  Called by every lane.
__device__ uint32_t block_scan(uint32_t* a, uint32_t n, uint32_t* tmp) {
    const uint32_t T = blockDim.x, t = threadIdx.x;
    const uint32_t per = (n + T - 1u) / T;
    const uint32_t i0 = umin(t * per, n), i1 = umin(i0 + per, n);
    uint32_t sum = 0u;
    for (uint32_t i = i0; i < i1; ++i) sum += a[i];
    tmp[t] = sum;
    __syncthreads();
    for (uint32_t d = 1u; d < T; d <<= 1) {
        const uint32_t v = t >= d ? tmp[t - d] : 0u;
        __syncthreads();
        tmp[t] += v;
        __syncthreads();
    }
    uint32_t run = tmp[t] - sum;
    const uint32_t total = tmp[T - 1u];
    for (uint32_t i = i0; i < i1; ++i) { const uint32_t v = a[i]; a[i] = run; run += v; }
    __syncthreads();
    return total;
}

// a sort's enumeration of positions: the plain form's is 0, 1, 2, ... (and the argument is empty); the dictionary form's is first,
// first + 1, ... with the three positions from gap_at on left out
template <bool DICT> struct Positions { uint32_t first = 0u, gap_at = NONE; };
template <> struct Positions<false> {};
__device__ __forceinline__ uint32_t nth(Positions<false>, uint32_t i) { return i; }
__device__ __forceinline__ uint32_t nth(Positions<true> ps, uint32_t i) {
    const uint32_t e = i + ps.first;
    return e >= ps.gap_at ? e + 3u : e;
}

// one stable counting pass of the sort: the elements src[0, np) (null: 0, 1, 2, ...) go to dst ordered by bits [shift, shift + 5) of
// their hash.  Segment s = [s * seglen, + seglen) has the counter column cnt[d * SEGS + s]: nobody else touches it.
template <bool DICT>
__device__ void sort_pass(const uint32_t* win, uint32_t mis, const uint16_t* src, uint16_t* dst, uint32_t np, uint32_t shift, uint32_t* cnt,
                          uint32_t* tmp, Positions<DICT> ps = {}) {
    const uint32_t seglen = (np + SEGS - 1u) / SEGS;
    for (uint32_t i = threadIdx.x; i < DIGITS * SEGS; i += blockDim.x) cnt[i] = 0u;
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < SEGS; s += blockDim.x) {
        const uint32_t i0 = umin(s * seglen, np), i1 = umin(i0 + seglen, np);
        for (uint32_t i = i0; i < i1; ++i) {
            const uint32_t e = src ? src[i] : nth(ps, i);
            cnt[((hash_of(ld32(win, mis + e)) >> shift) & (DIGITS - 1u)) * SEGS + s] += 1u;
        }
    }
    __syncthreads();
    block_scan(cnt, DIGITS * SEGS, tmp);
    for (uint32_t s = threadIdx.x; s < SEGS; s += blockDim.x) {
        const uint32_t i0 = umin(s * seglen, np), i1 = umin(i0 + seglen, np);
        for (uint32_t i = i0; i < i1; ++i) {
            const uint32_t e = src ? src[i] : nth(ps, i);
            const uint32_t c = ((hash_of(ld32(win, mis + e)) >> shift) & (DIGITS - 1u)) * SEGS + s;
            dst[cnt[c]] = (uint16_t)e;
            cnt[c] += 1u;
        }
    }
    __syncthreads();
}

// is position j of the chunk a literal?  L = its best length, next = best length of j + 1 (csize: the chunk's size).  PARSE 1: L is the
// length the optimal parse chose for j, and that is all there is to read
template <uint32_t PARSE = 0u>
__device__ __forceinline__ bool is_literal(uint32_t j, uint32_t L, uint32_t next, uint32_t csize) {
    if constexpr (PARSE != 0u) return L < 4u;
    return L < 4u || (j + 1u < csize && next > L);
}

// ---- "compress_parse" 1: the optimal parse (tests/sim/high_optimal_model.c), one wavefront per segment of SEG positions
constexpr uint32_t SEG = 2048u, SHORT_MAX = 35u;
constexpr uint32_t NO_CANDIDATE = 0x80000000u;
static_assert(2u * CHUNK0 <= L_BIG_END, "a cost (u16) per position of the chunk takes the window's LDS");

template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ uint32_t dpp_or(uint32_t old, uint32_t v) {      // v moved by CTRL; a lane without a source (or outside ROWS): old
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROWS, 0xf, false);
}
// the minimum over the wavefront's 64 lanes, as a uniform value
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    v = umin(v, dpp_or<0x111>(NONE, v));          // row_shr:1, 2, 4, 8: lane 15 of a row holds the row's minimum
    v = umin(v, dpp_or<0x112>(NONE, v));
    v = umin(v, dpp_or<0x114>(NONE, v));
    v = umin(v, dpp_or<0x118>(NONE, v));
    v = umin(v, dpp_or<0x142, 0xa>(NONE, v));     // row_bcast:15 into rows 1 and 3
    v = umin(v, dpp_or<0x143, 0xc>(NONE, v));     // row_bcast:31 into rows 2 and 3: lane 63 holds the wavefront's
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// blen[0, cn) (best[].len of the chunk's positions) becomes len'[]; cost: u16[cn] of LDS.  Called by every lane of the workgroup, between
// two barriers of the caller's.  Wavefront v takes the segments v, v + 16, ...: a segment reads and writes nothing of another one.
//   lane k holds w = CO(j + 1 + k), the cost behind a sequence of k + 1 bytes at j (0 from the segment's end on), and prices one
//   candidate: lane 0 the literal, lane l - 1 the match of l bytes -- a short one (4 <= l <= 35, l < L, l <= room) or the full one
//   (l == L <= 64); a full length above 64 is priced in lane 63 from cost[j + L] in LDS.  The step is the minimum of (cost << 6) | rank
//   (rank 0: the full length, 36 - l: a short one, 63: the literal -- the model's ties), then w moves up by one lane and lane 0
//   takes the new cost.
//   A segment goes in runs of 64 positions, lane i of a run = position jb + i: the lengths arrive, and the full length's price and the
//   short lengths' limit are worked out, for 64 positions at once; a step reads its three values by lane number and leaves its
//   minimum in lane i; the run's len'[] and costs are decoded and stored together.  (best[].len is 0 or at least 4.)
__device__ void optimal_lengths(uint16_t* blen, uint32_t cn, uint16_t* cost) {
    const uint32_t lane = threadIdx.x & 63u, l = lane + 1u;
    // what the lane's literal / short match adds to w << 6, and its length for the limit (the literal: 0, below every limit)
    const uint32_t own_add = lane == 0u ? (1u << 6) | 63u
                             : (l >= 4u && l <= SHORT_MAX) ? ((3u + (l >= 19u ? 1u : 0u)) << 6) | (SHORT_MAX + 1u - l) : NO_CANDIDATE;
    const uint32_t own_len = lane == 0u ? 0u : l;
    const uint32_t nwave = blockDim.x >> 6, nseg = (cn + SEG - 1u) / SEG;
    for (uint32_t sg = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); sg < nseg; sg += nwave) {
        const uint32_t s0 = sg * SEG, se = umin(s0 + SEG, cn);
        const uint32_t nb = (se - s0 + 63u) >> 6;
        uint32_t w = 0u;
        uint32_t Lnext = s0 + (nb - 1u) * 64u + lane < se ? blen[s0 + (nb - 1u) * 64u + lane] : 0u;
        for (uint32_t bk = nb; bk-- > 0u;) {
            const uint32_t jb = s0 + bk * 64u;
            const uint32_t Lv = Lnext;
            Lnext = bk ? blen[jb - 64u + lane] : 0u;
            const uint32_t roomv = se - (jb + lane);              // (lanes behind the segment's end: not read)
            const uint32_t Lpv = umin(Lv, roomv);
            const uint32_t fullv = (3u + ext_bytes(Lpv < 4u ? 0u : Lpv - 4u)) << 6;
            const uint32_t limv = max(umin(Lv, roomv + 1u), 1u);  // a short l: l < L and l <= room; the literal always
            uint32_t keyv = 0u;
            for (uint32_t i = umin(64u, se - jb); i-- > 0u;) {
                const uint32_t L = (uint32_t)__builtin_amdgcn_readlane((int)Lv, (int)i);
                const uint32_t full = (uint32_t)__builtin_amdgcn_readlane((int)fullv, (int)i);
                const uint32_t lim = (uint32_t)__builtin_amdgcn_readlane((int)limv, (int)i);
                uint32_t add = own_len < lim ? own_add : NO_CANDIDATE;
                add = l == L ? full : add;
                uint32_t key = (w << 6) + add;
                if (L > 64u) {                                    // (its cost lies in a run that is stored: j + L > jb + 63)
                    const uint32_t x = jb + i + L;
                    const uint32_t far = x < se ? cost[x] : 0u;
                    if (lane == 63u) key = (far << 6) + full;
                }
                const uint32_t m = wave_min(key);
                if (lane == i) keyv = m;
                w = dpp_or<0x138>(m >> 6, w);                     // wave_shr:1; lane 0 keeps the new cost
            }
            if (jb + lane < se) {
                const uint32_t r = keyv & 63u;
                blen[jb + lane] = (uint16_t)(r == 0u ? Lv : (r == 63u ? 0u : SHORT_MAX + 1u - r));
                cost[jb + lane] = (uint16_t)(keyv >> 6);
            }
        }
    }
}

// The dictionary form's stage of chunk 0: the window is the dictionary's last H bytes (they end at dend, any alignment) and the block's
// first blk bytes; window byte w is LDS byte mis + w with mis = (in - H) & 3, so the block's bytes arrive as aligned dwords.  A dword of
// the tail is two aligned dwords of the dictionary and a funnel shift; nothing is read outside the aligned dwords that hold the tail and
// the block, and the dword with bytes of both has one writer.
__device__ void stage_dict(uint32_t* win, uint32_t mis, const uint8_t* dend, uint32_t H, const uint8_t* in, uint32_t blk) {
    const uintptr_t d0 = (uintptr_t)dend - H;
    const uintptr_t lo_ok = d0 & ~(uintptr_t)3, hi_ok = ((uintptr_t)dend - 1u) & ~(uintptr_t)3;
    const uintptr_t a0 = d0 - mis;                               // where LDS byte 0 comes from
    const uint32_t sh = (uint32_t)(a0 & 3u);
    const uint32_t r = (mis + H) & 3u, jd = (mis + H) >> 2;      // the tail's bytes in the junction dword (0: none); the block's first dword
    const uint32_t* bsrc = (const uint32_t*)(in - r);
    const uint32_t ndw = (mis + H + blk + 3u) >> 2;
    for (uint32_t i = threadIdx.x; i < ndw; i += blockDim.x) {
        uint32_t v = 0u;
        if (4u * i < mis + H) {
            const uintptr_t p = (a0 & ~(uintptr_t)3) + 4u * (uintptr_t)i;
            const uint32_t lo = (p >= lo_ok && p <= hi_ok) ? *(const uint32_t*)p : 0u;
            const uint32_t hi = (sh != 0u && p + 4u >= lo_ok && p + 4u <= hi_ok) ? *(const uint32_t*)(p + 4u) : 0u;
            v = __builtin_amdgcn_alignbyte(hi, lo, sh);
        }
        if (i >= jd) {
            const uint32_t bv = bsrc[i - jd];
            const uint32_t keep = (i == jd && r != 0u) ? (1u << (8u * r)) - 1u : 0u;
            v = (v & keep) | (bv & ~keep);
        }
        win[i] = v;
    }
}

// DICT: the block has the dictionary that ends at dend, its last H bytes are chunk 0's history (H == 0: none; the plain form's bytes).
// dg_sorted / dg_start (nullable): the dictionary tail's digest (lz4_high_digest_kernel) -- chunk 0 sorts the block's positions only.
// HIST (with DICT): the dictionary is the block's own stream in front of it, dend == the block's start (the history form).
// PARSE: "compress_parse" -- 1 adds step 3 1/2 (optimal_lengths) and the walk reads its lengths without the lazy test.
template <bool DICT, bool HIST = false, uint32_t PARSE = 0u>
__device__ void compress_block(const CompressArgs& a, uint32_t b, uint8_t* lds, uint8_t* ws, uint32_t depth, const uint8_t* dend = nullptr,
                               uint32_t H_ = 0u, const uint16_t* dg_sorted = nullptr, const uint16_t* dg_start = nullptr) {
    const uint32_t T = blockDim.x, t = threadIdx.x;
    const uint32_t H = DICT ? H_ : 0u;
    const uint32_t n = a.in_len[b], cap = a.out_cap[b];
    const uint8_t* in = a.in_base + a.in_off[b];
    uint8_t* out = a.out_base + a.out_off[b];
    if ((uint64_t)cap < 20ull + (uint64_t)n * 110ull / 100ull) {      // get_maximum_output_size: the rule of every encoder here
        if (t == 0u) { a.out_len[b] = 0u; a.status[b] = LZ4FLEX_DEV_E_OUTPUT_TOO_SMALL; }
        return;
    }
    uint32_t* win = (uint32_t*)lds;
    uint32_t* cnt = (uint32_t*)(lds + L_CNT);
    uint16_t* exitd = (uint16_t*)lds;
    uint32_t* seqpos = (uint32_t*)(lds + L_SEQPOS);
    uint32_t* seqoff = (uint32_t*)(lds + L_SEQOFF);
    uint32_t* entry = (uint32_t*)(lds + L_ENTRY);
    uint32_t* tcnt = (uint32_t*)(lds + L_TCNT);
    uint32_t* tmp = (uint32_t*)(lds + L_TMP);
    uint32_t* misc = (uint32_t*)(lds + L_MISC);
    uint16_t* sort_a = (uint16_t*)(ws + W_SORT_A);
    uint16_t* sort_b = (uint16_t*)(ws + W_SORT_B);
    uint16_t* blen = (uint16_t*)(ws + W_LEN);
    uint16_t* boff = (uint16_t*)(ws + W_OFF);

    uint32_t anchor = 0u, opos = 0u;              // the same in every lane
    if (n >= 12u) for (uint32_t cs = 0u; cs + 12u <= n;) {
        // (with a dictionary chunk 0 is [0, CHUNK) and its window starts H bytes in front of the block: base = -H, in u32 arithmetic)
        const uint32_t ce = cs == 0u ? (H ? CHUNK : CHUNK0) : (cs + CHUNK < cs ? 0xFFFFFFFFu : cs + CHUNK);
        const uint32_t base = cs == 0u ? 0u - H : cs - CHUNK, hist = cs - base;
        const bool dchunk = DICT && cs == 0u && H != 0u;          // the window holds the dictionary's tail
        const bool use_dg = dchunk && dg_sorted != nullptr;
        const uint32_t end = umin(ce, n), mend = umin(ce, n - 5u);
        const uint32_t wlen = end - base;                         // the window's bytes
        const uint32_t np = umin(end, n - 11u) - base;            // ... and its positions with a hash (> hist)
        const uint32_t cn = end - cs, csize = ce - cs;            // the chunk's positions that exist; its size
        const uint32_t nh = np - hist;                            // ... and those with a hash

        // 1  stage (the aligned dwords that hold the window: the first and the last one may reach 3 bytes past it, inside their dword)
        const uint32_t mis = dchunk ? (uint32_t)(((uintptr_t)in - H) & 3u) : (uint32_t)((uintptr_t)(in + base) & 3u);
        if (!HIST && dchunk) stage_dict(win, mis, dend, H, in, end);
        else {                                                    // (HIST: the tail lies in front of the block -- one run of dwords)
            const uint32_t* src = (const uint32_t*)((HIST && dchunk ? in - H : in + base) - mis);
            const uint32_t ndw = (mis + wlen + 3u) >> 2;
            for (uint32_t i = t; i < ndw; i += T) win[i] = src[i];
        }
        if (t == 0u) misc[0] = 0u;
        __syncthreads();

        // 2  sort.  With a dictionary: without the three positions whose 4 bytes straddle its end; with its digest: the block's alone
        const uint32_t ns = use_dg ? nh : (dchunk ? np - 3u : np);
        Positions<DICT> ps;
        if constexpr (DICT) { ps.first = use_dg ? H : 0u; ps.gap_at = dchunk && !use_dg ? H - 3u : NONE; }
        sort_pass<DICT>(win, mis, nullptr, sort_a, ns, 0u, cnt, tmp, ps);
        sort_pass<DICT>(win, mis, sort_a, sort_b, ns, DIGIT_BITS, cnt, tmp);
        sort_pass<DICT>(win, mis, sort_b, sort_a, ns, 2u * DIGIT_BITS, cnt, tmp);

        // 3  match
        for (uint32_t j = nh + t; j <= cn; j += T) blen[j] = 0u;  // positions without a hash, and the one behind the block's end
        for (uint32_t i = t; i < ns; i += T) {
            const uint32_t e = sort_a[i];
            if (e < hist) continue;
            const uint32_t lim = mend - (base + e), x = mis + e;
            const uint32_t v = ld32(win, x), h = hash_of(v);
            uint32_t bl = 0u, bo = 0u;
            // (with a digest: behind the position's own left neighbours of its hash, the digest's bucket from its end downwards --
            // nearest first across both, the same `depth` and the same stop at the bucket's end)
            uint32_t own = i, dg = 0u, dg0 = 0u;
            bool in_own = true;
            if (use_dg) { dg0 = dg_start[h]; dg = dg_start[h + 1u]; }
            for (uint32_t k = 1u; k <= depth && (DICT || k <= i); ++k) {
                uint32_t q, c;
                if constexpr (!DICT) {
                    q = sort_a[i - k];
                    c = ld32(win, mis + q);
                    if (c != v) {
                        if (hash_of(c) != h) break;               // the bucket's end
                        continue;                                 // a collision: one of the `depth`
                    }
                } else {
                    bool have = false;
                    if (in_own && own != 0u) {
                        q = sort_a[--own];
                        c = ld32(win, mis + q);
                        have = c == v || hash_of(c) == h;
                    }
                    if (!have) {
                        in_own = false;
                        if (dg == dg0) break;                     // the bucket's end
                        q = dg_sorted[--dg];
                        c = ld32(win, mis + q);
                    }
                    if (c != v) continue;
                }
                const uint32_t y = mis + q;
                uint32_t l = 4u;
                bool open = true;
                while (l + 8u <= lim) {
                    const uint64_t d = ld64(win, x + l) ^ ld64(win, y + l);
                    if (d) { l += (uint32_t)__builtin_ctzll(d) >> 3; open = false; break; }
                    l += 8u;
                }
                if (open) while (l < lim && ld8(win, x + l) == ld8(win, y + l)) ++l;
                if (l > lim) l = lim;                             // (the chunk ends less than 4 bytes behind the position)
                if (l >= 4u && l > bl) { bl = l; bo = e - q; }
                if (bl == lim) break;                             // nothing is longer, and an equal one does not replace it
            }
            blen[e - hist] = (uint16_t)bl;
            boff[e - hist] = (uint16_t)bo;
        }
        __syncthreads();

        // 3 1/2  the optimal parse: best[].len becomes len'[] (the window's LDS is dead, the exits take it behind the barrier)
        if constexpr (PARSE != 0u) {
            optimal_lengths(blen, cn, (uint16_t*)lds);
            __syncthreads();
        }

        // 4  orbit.  exitd[j]: where the walk that enters its tile at j leaves it, counted from the tile's end
        const uint32_t ntile = (cn + TILE - 1u) / TILE;
        for (uint32_t tl = t; tl < ntile; tl += T) {
            const uint32_t ts = tl * TILE, te = umin(ts + TILE, cn);
            entry[tl] = NONE;
            uint32_t next = te < csize ? blen[te] : 0u;
            for (uint32_t j = te; j-- > ts;) {
                const uint32_t L = blen[j];
                const uint32_t nx = is_literal<PARSE>(j, L, next, csize) ? j + 1u : j + L;
                exitd[j] = (uint16_t)(nx >= te ? nx - te : exitd[nx]);
                next = L;
            }
        }
        __syncthreads();
        if (t == 0u) {
            for (uint32_t e = 0u; e < cn;) {
                const uint32_t tl = e / TILE;
                entry[tl] = e;
                e = umin(tl * TILE + TILE, cn) + exitd[e];
            }
        }
        __syncthreads();
        for (uint32_t tl = t; tl < ntile; tl += T) {
            const uint32_t te = umin(tl * TILE + TILE, cn);
            uint32_t c = 0u;
            if (entry[tl] != NONE)
                for (uint32_t j = entry[tl]; j < te;) {
                    const uint32_t L = blen[j];
                    if (is_literal<PARSE>(j, L, blen[j + 1u], csize)) ++j; else { ++c; j += L; }
                }
            tcnt[tl] = c;
        }
        __syncthreads();
        const uint32_t nseq = block_scan(tcnt, ntile, tmp);       // (the exits are dead from here on: the sequence lists take their LDS)
        for (uint32_t tl = t; tl < ntile; tl += T) {
            const uint32_t te = umin(tl * TILE + TILE, cn);
            uint32_t c = tcnt[tl];
            if (entry[tl] != NONE)
                for (uint32_t j = entry[tl]; j < te;) {
                    const uint32_t L = blen[j];
                    if (is_literal<PARSE>(j, L, blen[j + 1u], csize)) ++j; else { seqpos[c++] = j; j += L; }
                }
        }
        __syncthreads();

        // 5  sizes: sequence k = the literals since the match before it (the first one: since `anchor`) + its match
        for (uint32_t k = t; k < nseq; k += T) {
            const uint32_t j = seqpos[k], L = blen[j];
            const uint32_t from = k ? cs + seqpos[k - 1u] + blen[seqpos[k - 1u]] : anchor;
            const uint32_t lit = cs + j - from;
            seqoff[k] = 1u + ext_bytes(lit) + lit + 2u + ext_bytes(L - 4u);
        }
        __syncthreads();
        const uint32_t bytes = block_scan(seqoff, nseq, tmp);
        if ((uint64_t)opos + bytes > cap) {       // (cannot happen under the rule above: no store is ever made outside the slot)
            if (t == 0u) { a.out_len[b] = 0u; a.status[b] = LZ4FLEX_DEV_E_OUTPUT_TOO_SMALL; }
            return;
        }

        // 6  emit
        for (uint32_t k = t; k < nseq; k += T) {
            const uint32_t j = seqpos[k], L = blen[j], off = boff[j];
            const uint32_t from = k ? cs + seqpos[k - 1u] + blen[seqpos[k - 1u]] : anchor;
            const uint32_t lit = cs + j - from, ml = L - 4u;
            uint8_t* o = out + opos + seqoff[k];
            *o++ = (uint8_t)((umin(lit, 15u) << 4) | umin(ml, 15u));
            o = put_ext(o, lit);
            if (lit < LONG_LIT) for (uint32_t i = 0u; i < lit; ++i) o[i] = in[from + i];
            else misc[1u + atomicAdd(&misc[0], 1u)] = k;
            o += lit;
            *o++ = (uint8_t)off; *o++ = (uint8_t)(off >> 8);
            put_ext(o, ml);
        }
        __syncthreads();
        const uint32_t nlong = misc[0];
        for (uint32_t i = 0u; i < nlong; ++i) {
            const uint32_t k = misc[1u + i];
            const uint32_t from = k ? cs + seqpos[k - 1u] + blen[seqpos[k - 1u]] : anchor;
            const uint32_t lit = cs + seqpos[k] - from;
            uint8_t* o = out + opos + seqoff[k] + 1u + ext_bytes(lit);
            for (uint32_t x = t; x < lit; x += T) o[x] = in[from + x];
        }
        if (nseq) anchor = cs + seqpos[nseq - 1u] + blen[seqpos[nseq - 1u]];
        opos += bytes;
        __syncthreads();                          // (the next chunk's window overwrites the lists)
        if (ce >= n) break;
        cs = ce;
    }

    // the block's last literals
    const uint32_t lit = n - anchor;
    const uint64_t total = (uint64_t)opos + 1u + ext_bytes(lit) + lit;
    if (total > cap) {
        if (t == 0u) { a.out_len[b] = 0u; a.status[b] = LZ4FLEX_DEV_E_OUTPUT_TOO_SMALL; }
        return;
    }
    uint8_t* o = out + opos + 1u + ext_bytes(lit);
    if (t == 0u) {
        out[opos] = (uint8_t)(umin(lit, 15u) << 4);
        put_ext(out + opos + 1u, lit);
        a.out_len[b] = (uint32_t)total;
        a.status[b] = 0;
    }
    for (uint32_t x = t; x < lit; x += T) o[x] = in[anchor + x];
}

__global__ void __launch_bounds__(THREADS) lz4_compress_high_kernel(const CompressArgs a, uint8_t* ws, uint32_t depth) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[LDS_BYTES];
    for (uint32_t b = blockIdx.x; b < a.n; b += gridDim.x) {
        compress_block<false>(a, b, lds, ws + (size_t)blockIdx.x * WS_PER_WG, depth);
        __syncthreads();
    }
}
// ("compress_parse" 1 has three kernels of its own, each written like its parse 0 one: behind a shared body the compiler gives the
// parse 0 kernels other instruction streams than they had before the setting existed)
__global__ void __launch_bounds__(THREADS) lz4_compress_high_optimal_kernel(const CompressArgs a, uint8_t* ws, uint32_t depth) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[LDS_BYTES];
    for (uint32_t b = blockIdx.x; b < a.n; b += gridDim.x) {
        compress_block<false, false, 1u>(a, b, lds, ws + (size_t)blockIdx.x * WS_PER_WG, depth);
        __syncthreads();
    }
}

// The dictionary form ("compress_high_dict" 1; the bytes: tests/sim/high_dict_model.c).  Block b's dictionary is the set's (d.set),
// else the batch's one (d.shared), else a.dict_*; one of less than 4 bytes is none.  digest (nullable, with d.shared only): the slice
// lz4_high_digest_kernel filled.
__global__ void __launch_bounds__(THREADS) lz4_compress_high_dict_kernel(const CompressArgs a, const DictSource d, uint8_t* ws, const uint8_t* digest,
                                                                         uint32_t depth) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[LDS_BYTES];
    for (uint32_t b = blockIdx.x; b < a.n; b += gridDim.x) {
        // (block_dict's rule, lz4_device.h, written out: with the lookup in its place the compiler gives this kernel another instruction stream)
        const uint8_t* dict = nullptr;
        uint32_t dl = 0u;
        bool ok = true;
        if (d.has_set) ok = dict_set_find(d.set, b, dict, dl);
        else if (d.shared) { dict = d.shared; dl = d.shared_len; }
        else if (a.dict_len) {
            dl = a.dict_len[b];
            dict = a.dict_base + a.dict_off[b];
            ok = dl == 0u || a.flags == nullptr || a.flags[b] == 0u;      // a dictionary and frame flags or history bits: refused
        }
        if (!ok) {
            if (threadIdx.x == 0u) { a.out_len[b] = 0u; a.status[b] = LZ4FLEX_DEV_E_INVALID_ARG; }
            continue;
        }
        const uint32_t H = dl < 4u ? 0u : umin(dl, CHUNK);
        compress_block<true>(a, b, lds, ws + (size_t)blockIdx.x * WS_PER_WG, depth, dict + dl, H,
                             digest ? (const uint16_t*)(digest + W_SORT_A) : nullptr, (const uint16_t*)(digest + W_SORT_B));
        __syncthreads();
    }
}
__global__ void __launch_bounds__(THREADS) lz4_compress_high_dict_optimal_kernel(const CompressArgs a, const DictSource d, uint8_t* ws,
                                                                                 const uint8_t* digest, uint32_t depth) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[LDS_BYTES];
    for (uint32_t b = blockIdx.x; b < a.n; b += gridDim.x) {
        const uint8_t* dict = nullptr;                            // (the ladder of lz4_compress_high_dict_kernel)
        uint32_t dl = 0u;
        bool ok = true;
        if (d.has_set) ok = dict_set_find(d.set, b, dict, dl);
        else if (d.shared) { dict = d.shared; dl = d.shared_len; }
        else if (a.dict_len) {
            dl = a.dict_len[b];
            dict = a.dict_base + a.dict_off[b];
            ok = dl == 0u || a.flags == nullptr || a.flags[b] == 0u;
        }
        if (!ok) {
            if (threadIdx.x == 0u) { a.out_len[b] = 0u; a.status[b] = LZ4FLEX_DEV_E_INVALID_ARG; }
            continue;
        }
        const uint32_t H = dl < 4u ? 0u : umin(dl, CHUNK);
        compress_block<true, false, 1u>(a, b, lds, ws + (size_t)blockIdx.x * WS_PER_WG, depth, dict + dl, H,
                                        digest ? (const uint16_t*)(digest + W_SORT_A) : nullptr, (const uint16_t*)(digest + W_SORT_B));
        __syncthreads();
    }
}

// The history form ("compress_high_linked" 1): the dictionary form with block b's dictionary = the a.flags[b] >> 8 bytes of its own
// stream in front of it (LZ4FLEX_BLOCK_HISTORY; the low byte is not read).  It ends where the block starts, so chunk 0's window is one
// run of aligned dwords: no read leaves the dwords that hold [in - H, in + n).  a.flags is not null, a's dictionaries are not read.
__global__ void __launch_bounds__(THREADS) lz4_compress_high_linked_kernel(const CompressArgs a, uint8_t* ws, uint32_t depth) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[LDS_BYTES];
    for (uint32_t b = blockIdx.x; b < a.n; b += gridDim.x) {
        const uint32_t h = a.flags[b] >> 8;
        const uint32_t H = h < 4u ? 0u : umin(h, CHUNK);
        compress_block<true, true>(a, b, lds, ws + (size_t)blockIdx.x * WS_PER_WG, depth, a.in_base + a.in_off[b], H);
        __syncthreads();
    }
}
__global__ void __launch_bounds__(THREADS) lz4_compress_high_linked_optimal_kernel(const CompressArgs a, uint8_t* ws, uint32_t depth) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[LDS_BYTES];
    for (uint32_t b = blockIdx.x; b < a.n; b += gridDim.x) {
        const uint32_t h = a.flags[b] >> 8;
        const uint32_t H = h < 4u ? 0u : umin(h, CHUNK);
        compress_block<true, true, 1u>(a, b, lds, ws + (size_t)blockIdx.x * WS_PER_WG, depth, a.in_base + a.in_off[b], H);
        __syncthreads();
    }
}

// The digest of one dictionary's tail: its hashed positions (q + 4 <= H) in the order the joint sort gives them, and the buckets' bounds.
// One workgroup; `slice` is a workgroup's slice of the workspace: u16 sorted[H - 3] at W_SORT_A, u16 start[32 769] at W_SORT_B (the
// positions with hash h are sorted[start[h] .. start[h + 1])).  len >= 4.
__global__ void __launch_bounds__(THREADS) lz4_high_digest_kernel(const uint8_t* dict, uint32_t len, uint8_t* slice) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[LDS_BYTES];
    const uint32_t T = blockDim.x, t = threadIdx.x;
    uint32_t* win = (uint32_t*)lds;
    uint32_t* cnt = (uint32_t*)(lds + L_CNT);
    uint32_t* tmp = (uint32_t*)(lds + L_TMP);
    uint16_t* sort_a = (uint16_t*)(slice + W_SORT_A);
    uint16_t* sort_b = (uint16_t*)(slice + W_SORT_B);
    const uint32_t H = umin(len, CHUNK), np = H - 3u;
    const uint8_t* tail = dict + (len - H);
    const uint32_t mis = (uint32_t)((uintptr_t)tail & 3u);
    {
        const uint32_t* src = (const uint32_t*)(tail - mis);
        const uint32_t ndw = (mis + H + 3u) >> 2;
        for (uint32_t i = t; i < ndw; i += T) win[i] = src[i];
    }
    __syncthreads();
    sort_pass<false>(win, mis, nullptr, sort_a, np, 0u, cnt, tmp);
    sort_pass<false>(win, mis, sort_a, sort_b, np, DIGIT_BITS, cnt, tmp);
    sort_pass<false>(win, mis, sort_b, sort_a, np, 2u * DIGIT_BITS, cnt, tmp);
    __threadfence_block();
    __syncthreads();
    uint16_t* start = sort_b;                     // (the second array is dead behind the last pass)
    for (uint32_t i = t; i <= np; i += T) {
        const uint32_t h0 = i ? hash_of(ld32(win, mis + sort_a[i - 1u])) + 1u : 0u;
        const uint32_t h1 = i < np ? hash_of(ld32(win, mis + sort_a[i])) : 1u << HASH_BITS;
        for (uint32_t h = h0; h <= h1; ++h) start[h] = (uint16_t)i;
    }
}

}  // namespace high

size_t compress_high_workspace_bytes(int n_workgroups) { return (size_t)n_workgroups * high::WS_PER_WG; }

hipError_t launch_compress_high(const CompressArgs& a, void* workspace, size_t workspace_bytes, int max_workgroups, uint32_t depth, uint32_t parse, hipStream_t s) {
    if (a.n == 0u) return hipSuccess;
    const size_t fit = workspace_bytes / high::WS_PER_WG;
    const uint32_t g = (uint32_t)std::min<size_t>(std::min<size_t>(a.n, fit), (size_t)(max_workgroups > 0 ? max_workgroups : 0));
    if (g == 0u || depth == 0u || parse > 1u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(parse ? high::lz4_compress_high_optimal_kernel : high::lz4_compress_high_kernel, dim3(g), dim3(high::THREADS), 0, s, a, (uint8_t*)workspace, depth);
    return hipGetLastError();
}

hipError_t launch_compress_high_linked(const CompressArgs& a, void* workspace, size_t workspace_bytes, int max_workgroups, uint32_t depth,
                                       uint32_t parse, hipStream_t s) {
    if (a.n == 0u) return hipSuccess;
    const size_t fit = workspace_bytes / high::WS_PER_WG;
    const uint32_t g = (uint32_t)std::min<size_t>(std::min<size_t>(a.n, fit), (size_t)(max_workgroups > 0 ? max_workgroups : 0));
    if (g == 0u || depth == 0u || parse > 1u || a.flags == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(parse ? high::lz4_compress_high_linked_optimal_kernel : high::lz4_compress_high_linked_kernel, dim3(g), dim3(high::THREADS), 0, s, a, (uint8_t*)workspace, depth);
    return hipGetLastError();
}

hipError_t launch_compress_high_dict(const CompressArgs& a, const DictSource& d, bool use_digest, void* workspace, size_t workspace_bytes,
                                     int max_workgroups, uint32_t depth, uint32_t parse, hipStream_t s) {
    if (a.n == 0u) return hipSuccess;
    // the digest is a property of the batch's ONE dictionary; it takes the last slice of the workspace
    const bool dg = use_digest && !d.has_set && d.shared != nullptr && d.shared_len >= 4u;
    size_t fit = workspace_bytes / high::WS_PER_WG;
    if (dg && fit) --fit;
    const uint32_t g = (uint32_t)std::min<size_t>(std::min<size_t>(a.n, fit), (size_t)(max_workgroups > 0 ? max_workgroups : 0));
    if (g == 0u || depth == 0u || parse > 1u) return hipErrorInvalidValue;
    uint8_t* digest = dg ? (uint8_t*)workspace + fit * high::WS_PER_WG : nullptr;
    if (dg) {
        hipLaunchKernelGGL(high::lz4_high_digest_kernel, dim3(1), dim3(high::THREADS), 0, s, d.shared, d.shared_len, digest);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(parse ? high::lz4_compress_high_dict_optimal_kernel : high::lz4_compress_high_dict_kernel, dim3(g), dim3(high::THREADS), 0, s, a, d, (uint8_t*)workspace, (const uint8_t*)digest, depth);
    return hipGetLastError();
}

}  // namespace lz4flex_dev
