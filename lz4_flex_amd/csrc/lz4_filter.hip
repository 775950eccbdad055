// lz4_filter.hip -- the byte- and bit-shuffle filters of typed batches (lz4flex_filter_batch, lz4flex_compress_batch_typed,
// lz4flex_decompress_batch_typed; the definitions: include/lz4flex_amd.h "typed batches").  A block of L bytes with elements of E bytes:
//   SHUFFLE     m = L / E:            out[j * m + e] = in[e * E + j]                                  (e < m, j < E)
//   BITSHUFFLE  m8 = L / E / 8 * 8:   bit b of out[(8 j + k) * m8 / 8 + q] = bit k of in[(8 q + b) * E + j]   (q < m8 / 8, b, k < 8)
// and the bytes behind m * E / m8 * E stay where they are.  Four kernels -- shuffle, unshuffle, bitshuffle, unbitshuffle -- an instance per
// E, and a copy (FILTER_NONE; SHUFFLE with E = 1).
//
// WORK ITEMS are (block, tile) pairs, a wavefront per item, without a scan over the lengths: with W wavefronts in the grid and n blocks
// every block has P = max(1, W / n) of them, which take its tiles t = sub, sub + P, ... -- 65 536 blocks of one tile keep every wavefront
// busy (P = 1) and so does one block of 8 192 tiles (P = W).  What bounds it: a batch of one long block among many short ones leaves the
// long one to P wavefronts.
//
// A TILE is 1 024 elements: a lane takes 16 consecutive elements (16 E bytes, 16-byte loads), regroups them in registers (v_perm_b32)
// into 16 bytes per byte plane and
//   shuffle:     stores those 16 bytes: a wavefront step writes 1 KiB contiguous to each of the E planes;
//   bitshuffle:  transposes each plane's two 8 x 8 bit matrices (8 elements x 8 bits) and has 2 bytes for each of the 8 E bit planes;
//                the wavefront's 128 bytes per bit plane meet in LDS (1 024 E bytes per wavefront), from where lane r stores 16 of them
//                per round: E rounds, each 128 contiguous bytes to each of 8 bit planes.
// The inverses run the same steps backwards (plane loads of 16 bytes, 16 E contiguous bytes stored per lane).
//
// ALIGNMENT.  Every 16-byte STORE is 16-byte aligned; loads take any address (global memory does; lz4_copy_range.h does the same) and
// never leave [off, off + L).  A block whose stores cannot all be aligned -- the planes' starts differ mod 16 (shuffle: m % 16 != 0,
// bitshuffle: m8 / 8 % 16 != 0), an output the elements do not line up with -- and every block under "filter_bytewise" 1 goes by the
// narrow path: byte accesses, a lane per output byte.  So do the head in front of the first aligned store and the tail behind the last
// whole lane (tile 0's wavefront takes both, and the bytes behind the last element).
// All offsets are 64-bit.  Every store is a plain vector store.
//
// DELTA (LZ4FLEX_FILTER_DELTA, a template parameter beside KIND and E; the DELTA = false kernels are the ones above, instruction for
// instruction).  Forward, d[e] = x[e] - x[e - 1] mod 2^(8 E), d[e] = x[e] at every e % 1 024 == 0, goes in front of the base filter;
// the inverse sums d back to the restart behind it.  The restart is what keeps a tile's work in its wavefront: no scan over the block, no
// look-back between workgroups, no workspace, still one launch per pass.
//   forward:  a lane differences the 16 elements it loaded in registers (lz4_filter_delta.h: SWAR bytes for E = 1, packed halves for E = 2,
//             subtract with borrow over two dwords for E = 8) before to_planes; the element in front of its first comes from `in` (the
//             neighbouring lane has just loaded that line), and because the first aligned store lies up to 15 elements into the block,
//             the restart can be any of the 16.
//   inverse:  after from_planes a lane scans its 16 elements inclusively, the lanes' totals are summed exclusively over the wavefront (six
//             DPP row operations, no LDS; 64-bit for E = 8) and every lane adds its carry and stores.  A wide inverse tile is elements [1 024 t,
//             1 024 t + 1 024), exactly one restart segment, so nothing is segmented.  That needs tiles that start on a restart: a block
//             whose `out` is not 16-byte aligned (unshuffle tiles would start h elements in) goes by the NARROW path; every block whose
//             `out` is 16-byte aligned takes the wide one.
//   FILTER_NONE | DELTA (and SHUFFLE | DELTA at E = 1) are K_DELTA / K_UNDELTA: the same lanes with 16-byte loads and stores and no planes.
//   narrow:   forward, src_byte() is a byte of d[e] from x[e] and x[e - 1] wherever the base filter reads a byte of element e; the inverse
//             is undelta_narrow_tile: a wavefront per restart segment, a lane gathers its 16 consecutive d from wherever the base filter
//             put them (twice: once for its total, once to store the running sum byte by byte).  It never reads what this launch stored
//             -- the tail behind a wide block's last whole lane re-sums its segment from `in`.  The bit-shuffle's residue behind m8 is
//             differenced and summed like every other element, in place.
// Registers of the DELTA kernels: DESIGN.md "Delta stage"; none uses scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4_copy_range.h"
#include "lz4_device.h"
#include "lz4_filter_delta.h"

namespace lz4flex_dev {

namespace {

constexpr uint32_t THREADS = 256u;                       // four wavefronts, each on its own items
constexpr uint32_t WAVES = THREADS / 64u;
constexpr uint32_t TILE = FILTER_TILE_ELEMS;             // elements per (block, tile) item
constexpr uint32_t LANE_ELEMS = 16u;
static_assert(TILE == 64u * LANE_ELEMS, "a tile is one wavefront step of 16 elements per lane");
constexpr uint32_t COPY_TILE = 16384u;                   // bytes per item of the copy
constexpr uint32_t GRID = 2048u;                         // workgroups per launch (256 CUs x 8); the items stride over what is left

enum : int { K_SHUFFLE = 0, K_UNSHUFFLE = 1, K_BITSHUFFLE = 2, K_UNBITSHUFFLE = 3, K_COPY = 4, K_DELTA = 5, K_UNDELTA = 6 };
using lz4flex_delta::RESTART;
static_assert(RESTART == TILE, "a narrow tile, and an inverse tile of the wide path, is one restart segment");

__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }

// the 4 x 4 byte transpose: c[j] = {r[0].byte j, r[1].byte j, r[2].byte j, r[3].byte j}
__device__ __forceinline__ void tr4(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3) {
    const uint32_t x0 = perm(r1, r0, 0x05010400u), x1 = perm(r1, r0, 0x07030602u);
    const uint32_t y0 = perm(r3, r2, 0x05010400u), y1 = perm(r3, r2, 0x07030602u);
    c0 = perm(y0, x0, 0x05040100u); c1 = perm(y0, x0, 0x07060302u);
    c2 = perm(y1, x1, 0x05040100u); c3 = perm(y1, x1, 0x07060302u);
}

// 16 elements (w: 4 E words) -> 16 bytes per byte plane (pl[4 j + d]: byte j of elements 4 d .. 4 d + 3)
template <int E>
__device__ __forceinline__ void to_planes(const uint32_t* w, uint32_t* pl) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        if constexpr (E == 1) {
            pl[d] = w[d];
        } else if constexpr (E == 2) {
            pl[d] = perm(w[2 * d + 1], w[2 * d], 0x06040200u);
            pl[4 + d] = perm(w[2 * d + 1], w[2 * d], 0x07050301u);
        } else if constexpr (E == 4) {
            tr4(w[4 * d], w[4 * d + 1], w[4 * d + 2], w[4 * d + 3], pl[d], pl[4 + d], pl[8 + d], pl[12 + d]);
        } else {
            tr4(w[8 * d], w[8 * d + 2], w[8 * d + 4], w[8 * d + 6], pl[d], pl[4 + d], pl[8 + d], pl[12 + d]);
            tr4(w[8 * d + 1], w[8 * d + 3], w[8 * d + 5], w[8 * d + 7], pl[16 + d], pl[20 + d], pl[24 + d], pl[28 + d]);
        }
    }
}
template <int E>
__device__ __forceinline__ void from_planes(const uint32_t* pl, uint32_t* w) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        if constexpr (E == 1) {
            w[d] = pl[d];
        } else if constexpr (E == 2) {
            w[2 * d] = perm(pl[4 + d], pl[d], 0x05010400u);
            w[2 * d + 1] = perm(pl[4 + d], pl[d], 0x07030602u);
        } else if constexpr (E == 4) {
            tr4(pl[d], pl[4 + d], pl[8 + d], pl[12 + d], w[4 * d], w[4 * d + 1], w[4 * d + 2], w[4 * d + 3]);
        } else {
            tr4(pl[d], pl[4 + d], pl[8 + d], pl[12 + d], w[8 * d], w[8 * d + 2], w[8 * d + 4], w[8 * d + 6]);
            tr4(pl[16 + d], pl[20 + d], pl[24 + d], pl[28 + d], w[8 * d + 1], w[8 * d + 3], w[8 * d + 5], w[8 * d + 7]);
        }
    }
}

// the 8 x 8 bit transpose of x (byte i, bit k) -> (byte k, bit i); its own inverse
__device__ __forceinline__ uint64_t bit_tr8(uint64_t x) {
    uint64_t t;
    t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAull; x ^= t ^ (t << 7);
    t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCull; x ^= t ^ (t << 14);
    t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ull; x ^= t ^ (t << 28);
    return x;
}

__device__ __forceinline__ u32x4 load16(const uint8_t* p) { u32x4 v; __builtin_memcpy(&v, p, 16); return v; }      // any address
__device__ __forceinline__ void store16(uint8_t* p, u32x4 v) { *reinterpret_cast<u32x4*>(p) = v; }                 // 16-byte aligned
__device__ __forceinline__ void wave_sync() {           // LDS written by other lanes of this wavefront is read behind this
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ---- the delta stage's pieces (DELTA kernels only) ---------------------------------------------------------------------------------
template <int E>
__device__ __forceinline__ uint64_t load_elem(const uint8_t* p) {            // any address
    uint64_t v = 0u;
    __builtin_memcpy(&v, p, E);
    return v;
}
template <int E>
__device__ __forceinline__ void store_elem_bytes(uint8_t* p, uint64_t v) {
#pragma unroll
    for (int j = 0; j < E; ++j) p[j] = (uint8_t)(v >> (8 * j));
}
// d[e] of a block (its low E bytes)
template <int E>
__device__ __forceinline__ uint64_t delta_elem(const uint8_t* in, uint64_t e) {
    const uint64_t x = load_elem<E>(in + e * E);
    return (e & (RESTART - 1u)) ? x - load_elem<E>(in + (e - 1u) * E) : x;
}
// byte j of what the base filter reads as element e: x[e], or d[e] behind the delta stage
template <int E, bool DELTA>
__device__ __forceinline__ uint8_t src_byte(const uint8_t* in, uint64_t e, int j) {
    if constexpr (DELTA) return (uint8_t)(delta_elem<E>(in, e) >> (8 * j));
    else return in[e * E + j];
}
// the 16 elements at e0 of a lane of a forward kernel: x -> d
template <int E>
__device__ __forceinline__ void lane_delta(const uint8_t* in, uint64_t e0, uint32_t* w) {
    const uint64_t prev = e0 ? load_elem<E>(in + (e0 - 1u) * E) : 0u;
    lz4flex_delta::delta16<E>(w, prev, lz4flex_delta::restart_index(e0));
}
// v of the lane a DPP control names, 0 where there is none or the row / bank masks leave the lane out (bound_ctrl off: `old` = 0 stays)
template <int CTRL, int ROWS = 0xF, int BANKS = 0xF>
__device__ __forceinline__ uint32_t dpp(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, BANKS, false); }
template <int CTRL, int ROWS = 0xF, int BANKS = 0xF>
__device__ __forceinline__ uint64_t dpp(uint64_t v) {
    return (uint64_t)dpp<CTRL, ROWS, BANKS>((uint32_t)v) | ((uint64_t)dpp<CTRL, ROWS, BANKS>((uint32_t)(v >> 32)) << 32);
}
// the sum of `total` over the lanes in front of this one (mod 2^64; E < 8: mod 2^32), in DPP row operations: an inclusive scan of each
// row of 16 lanes (row_shr 1, 2, 4, 8), lane 15 of every row into rows 1 and 3 (row_bcast:15), lane 31 into rows 2 and 3 (row_bcast:31),
// less the lane's own.  A lane takes in only lanes below itself, so a prefix of the wavefront's lanes may run it alone.
template <typename T>
__device__ __forceinline__ T wave_inclusive_sum(T v) {
    v += dpp<0x111>(v);
    v += dpp<0x112>(v);
    v += dpp<0x114>(v);
    v += dpp<0x118>(v);
    v += dpp<0x142, 0xA>(v);
    v += dpp<0x143, 0xC>(v);
    return v;
}
template <int E>
__device__ __forceinline__ uint64_t wave_exclusive_sum(uint64_t total, uint32_t lane) {
    if constexpr (E < 8) return wave_inclusive_sum((uint32_t)total) - (uint32_t)total;
    else return wave_inclusive_sum(total) - total;
}
// d[e] as the base filter BASE laid it out in a filtered block of m elements
template <int BASE, int E>
__device__ __forceinline__ uint64_t filtered_elem(const uint8_t* in, uint64_t m, uint64_t e) {
    if constexpr (BASE == FILTER_SHUFFLE) {
        uint64_t v = 0u;
#pragma unroll
        for (int j = 0; j < E; ++j) v |= (uint64_t)in[(uint64_t)j * m + e] << (8 * j);
        return v;
    } else if constexpr (BASE == FILTER_BITSHUFFLE) {
        const uint64_t nb = m >> 3;
        if (e >= nb * 8u) return load_elem<E>(in + e * E);            // the residue behind m8 lies where it was
        const uint64_t q = e >> 3;
        const uint32_t bit = (uint32_t)e & 7u;
        uint64_t v = 0u;
        for (int p = 0; p < 8 * E; ++p) v |= (uint64_t)((in[(uint64_t)p * nb + q] >> bit) & 1u) << p;
        return v;
    } else {
        return load_elem<E>(in + e * E);
    }
}
// the narrow inverse of DELTA | BASE: restart segment tt (elements [1 024 tt, ...) below m) by one wavefront, a lane on 16 consecutive
// elements -- their sum, the wavefront's exclusive sums, then the running sums byte by byte to out; only elements >= lo are stored (the
// tail of a wide block needs the sums of elements that wide lanes store).  d is read from `in` twice, nothing is read from `out`.
template <int BASE, int E>
__device__ __forceinline__ void undelta_narrow_tile(const uint8_t* in, uint8_t* out, uint64_t m, uint64_t tt, uint64_t lo, uint32_t lane) {
    const uint64_t a = tt * TILE, b = a + TILE < m ? a + TILE : m;
    const uint64_t e0 = a + (uint64_t)lane * LANE_ELEMS;
    uint64_t total = 0u;
    for (uint32_t i = 0; i < LANE_ELEMS; ++i)
        if (e0 + i < b) total += filtered_elem<BASE, E>(in, m, e0 + i);
    uint64_t run = wave_exclusive_sum<E>(total, lane);
    for (uint32_t i = 0; i < LANE_ELEMS; ++i) {
        const uint64_t e = e0 + i;
        if (e < b) {
            run += filtered_elem<BASE, E>(in, m, e);
            if (e >= lo) store_elem_bytes<E>(out + e * E, run);
        }
    }
}
// elements [lo, m) of a block through undelta_narrow_tile, segment by segment (uniform over the wavefront)
template <int BASE, int E>
__device__ __forceinline__ void undelta_narrow_from(const uint8_t* in, uint8_t* out, uint64_t m, uint64_t lo, uint32_t lane) {
    if (lo >= m) return;
    for (uint64_t tt = lo / TILE; tt * TILE < m; ++tt) undelta_narrow_tile<BASE, E>(in, out, m, tt, lo, lane);
}
// forward, elements [a, b) in place (FILTER_NONE | DELTA; the bit-shuffle's residue): a lane per element
template <int E>
__device__ __forceinline__ void delta_narrow(const uint8_t* in, uint8_t* out, uint64_t a, uint64_t b, uint32_t lane) {
    for (uint64_t e = a + lane; e < b; e += 64u) store_elem_bytes<E>(out + e * E, delta_elem<E>(in, e));
}

// ---- the narrow path: a lane per output byte, the bytes of a plane over consecutive lanes ------------------------------------------
template <int E, bool DELTA = false>
__device__ __forceinline__ void shuffle_narrow(const uint8_t* in, uint8_t* out, uint64_t m, uint64_t a, uint64_t b, uint32_t lane) {
    for (int j = 0; j < E; ++j)
        for (uint64_t e = a + lane; e < b; e += 64u) out[(uint64_t)j * m + e] = src_byte<E, DELTA>(in, e, j);
}
template <int E>
__device__ __forceinline__ void unshuffle_narrow(const uint8_t* in, uint8_t* out, uint64_t m, uint64_t a, uint64_t b, uint32_t lane) {
    for (int j = 0; j < E; ++j)
        for (uint64_t e = a + lane; e < b; e += 64u) out[e * E + j] = in[(uint64_t)j * m + e];
}
// plane bytes q in [qa, qb) of every bit plane (nb = m8 / 8 bytes per plane)
template <int E, bool DELTA = false>
__device__ __forceinline__ void bitshuffle_narrow(const uint8_t* in, uint8_t* out, uint64_t nb, uint64_t qa, uint64_t qb, uint32_t lane) {
    for (int p = 0; p < 8 * E; ++p) {
        const int j = p >> 3, k = p & 7;
        for (uint64_t q = qa + lane; q < qb; q += 64u) {
            uint32_t v = 0u;
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) v |= (((uint32_t)src_byte<E, DELTA>(in, 8u * q + bit, j) >> k) & 1u) << bit;
            out[(uint64_t)p * nb + q] = (uint8_t)v;
        }
    }
}
// elements [8 qa, 8 qb)
template <int E>
__device__ __forceinline__ void unbitshuffle_narrow(const uint8_t* in, uint8_t* out, uint64_t nb, uint64_t qa, uint64_t qb, uint32_t lane) {
    for (int j = 0; j < E; ++j)
        for (uint64_t e = 8u * qa + lane; e < 8u * qb; e += 64u) {
            const uint64_t q = e >> 3;
            const uint32_t bit = (uint32_t)e & 7u;
            uint32_t v = 0u;
#pragma unroll
            for (int k = 0; k < 8; ++k) v |= (((uint32_t)in[(uint64_t)(8 * j + k) * nb + q] >> bit) & 1u) << k;
            out[e * E + j] = (uint8_t)v;
        }
}
__device__ __forceinline__ void copy_bytes(const uint8_t* in, uint8_t* out, uint64_t a, uint64_t b, uint32_t lane) {
    for (uint64_t i = a + lane; i < b; i += 64u) out[i] = in[i];
}

__device__ __forceinline__ uint64_t tiles_of(uint64_t items, uint64_t per) { const uint64_t t = (items + per - 1u) / per; return t ? t : 1u; }

// ---- one block, this wavefront's tiles sub, sub + P, ... ----------------------------------------------------------------------------
template <int E, bool DELTA>
__device__ __forceinline__ void shuffle_block(const uint8_t* in, uint8_t* out, uint64_t L, uint64_t sub, uint64_t P, uint32_t lane, bool bytewise) {
    const uint64_t m = L / E;
    if (bytewise || (m & 15u) != 0u) {
        const uint64_t nt = tiles_of(m, TILE);
        for (uint64_t t = sub; t < nt; t += P) {
            const uint64_t a = t * TILE, b = a + TILE < m ? a + TILE : m;
            shuffle_narrow<E, DELTA>(in, out, m, a, b, lane);
            if (t == 0u) copy_bytes(in, out, m * E, L, lane);
        }
        return;
    }
    // m % 16 == 0: every plane starts at the output's phase; h elements in front of the first aligned 16 bytes of a plane
    uint64_t h = (16u - ((uintptr_t)out & 15u)) & 15u;
    if (h > m) h = m;
    const uint64_t G = (m - h) / LANE_ELEMS;            // whole lanes
    const uint64_t nt = tiles_of(G, 64u);
    for (uint64_t t = sub; t < nt; t += P) {
        const uint64_t g = t * 64u + lane;
        if (g < G) {
            const uint64_t e0 = h + g * LANE_ELEMS;
            uint32_t w[4 * E], pl[4 * E];
#pragma unroll
            for (int v = 0; v < E; ++v) {
                const u32x4 x = load16(in + e0 * E + 16u * v);
                w[4 * v] = x.x; w[4 * v + 1] = x.y; w[4 * v + 2] = x.z; w[4 * v + 3] = x.w;
            }
            if constexpr (DELTA) lane_delta<E>(in, e0, w);
            to_planes<E>(w, pl);
#pragma unroll
            for (int j = 0; j < E; ++j) store16(out + (uint64_t)j * m + e0, u32x4{pl[4 * j], pl[4 * j + 1], pl[4 * j + 2], pl[4 * j + 3]});
        }
        if (t == 0u) {
            shuffle_narrow<E, DELTA>(in, out, m, 0u, h, lane);
            shuffle_narrow<E, DELTA>(in, out, m, h + G * LANE_ELEMS, m, lane);
            copy_bytes(in, out, m * E, L, lane);
        }
    }
}

template <int E, bool DELTA>
__device__ __forceinline__ void unshuffle_block(const uint8_t* in, uint8_t* out, uint64_t L, uint64_t sub, uint64_t P, uint32_t lane, bool bytewise) {
    const uint64_t m = L / E;
    // the elements do not line up with 16-byte stores; DELTA: a tile has to start on a restart, so no head: `out` 16-byte aligned
    if (bytewise || ((uintptr_t)out & (DELTA ? 15u : E - 1u)) != 0u) {
        const uint64_t nt = tiles_of(m, TILE);
        for (uint64_t t = sub; t < nt; t += P) {
            const uint64_t a = t * TILE, b = a + TILE < m ? a + TILE : m;
            if constexpr (DELTA) undelta_narrow_tile<FILTER_SHUFFLE, E>(in, out, m, t, 0u, lane);
            else unshuffle_narrow<E>(in, out, m, a, b, lane);
            if (t == 0u) copy_bytes(in, out, m * E, L, lane);
        }
        return;
    }
    uint64_t h = ((16u - ((uintptr_t)out & 15u)) & 15u) / E;        // elements in front of the first aligned 16 bytes
    if (h > m) h = m;
    const uint64_t G = (m - h) / LANE_ELEMS;
    const uint64_t nt = tiles_of(G, 64u);
    for (uint64_t t = sub; t < nt; t += P) {
        const uint64_t g = t * 64u + lane;
        if (g < G) {
            const uint64_t e0 = h + g * LANE_ELEMS;
            uint32_t w[4 * E], pl[4 * E];
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const u32x4 x = load16(in + (uint64_t)j * m + e0);
                pl[4 * j] = x.x; pl[4 * j + 1] = x.y; pl[4 * j + 2] = x.z; pl[4 * j + 3] = x.w;
            }
            from_planes<E>(pl, w);
            if constexpr (DELTA) lz4flex_delta::carry16<E>(w, wave_exclusive_sum<E>(lz4flex_delta::scan16<E>(w), lane));      // (h = 0: lane 0 starts a segment)
#pragma unroll
            for (int v = 0; v < E; ++v) store16(out + e0 * E + 16u * v, u32x4{w[4 * v], w[4 * v + 1], w[4 * v + 2], w[4 * v + 3]});
        }
        if (t == 0u) {
            if constexpr (DELTA) {
                undelta_narrow_from<FILTER_SHUFFLE, E>(in, out, m, G * LANE_ELEMS, lane);
            } else {
                unshuffle_narrow<E>(in, out, m, 0u, h, lane);
                unshuffle_narrow<E>(in, out, m, h + G * LANE_ELEMS, m, lane);
            }
            copy_bytes(in, out, m * E, L, lane);
        }
    }
}

// lds: this wavefront's 1 024 E bytes, bit plane p's 128 bytes of the tile at lds + 128 p
template <int E, bool DELTA>
__device__ __forceinline__ void bitshuffle_block(const uint8_t* in, uint8_t* out, uint64_t L, uint64_t sub, uint64_t P, uint32_t lane, bool bytewise,
                                                 uint8_t* lds) {
    const uint64_t nb = L / E / 8u;                      // bytes per bit plane
    const uint64_t body = nb * 8u * E;
    if (bytewise || (nb & 15u) != 0u) {
        const uint64_t nt = tiles_of(nb, TILE / 8u);
        for (uint64_t t = sub; t < nt; t += P) {
            const uint64_t a = t * (TILE / 8u), b = a + TILE / 8u < nb ? a + TILE / 8u : nb;
            bitshuffle_narrow<E, DELTA>(in, out, nb, a, b, lane);
            if (t == 0u) {
                if constexpr (DELTA) delta_narrow<E>(in, out, nb * 8u, L / E, lane);      // the residue is differenced where it lies
                copy_bytes(in, out, DELTA ? L / E * E : body, L, lane);
            }
        }
        return;
    }
    // nb % 16 == 0: every bit plane starts at the output's phase; hq plane bytes in front of the first aligned 16
    uint64_t hq = (16u - ((uintptr_t)out & 15u)) & 15u;
    if (hq > nb) hq = nb;
    const uint64_t C = (nb - hq) / 16u;                  // whole 16-byte chunks per plane = 128 elements = 8 lanes
    const uint64_t nt = tiles_of(C, 8u);
    for (uint64_t t = sub; t < nt; t += P) {
        const uint64_t g = t * 64u + lane;
        if ((g >> 3) < C) {
            const uint64_t e0 = 8u * hq + g * LANE_ELEMS;
            uint32_t w[4 * E], pl[4 * E];
#pragma unroll
            for (int v = 0; v < E; ++v) {
                const u32x4 x = load16(in + e0 * E + 16u * v);
                w[4 * v] = x.x; w[4 * v + 1] = x.y; w[4 * v + 2] = x.z; w[4 * v + 3] = x.w;
            }
            if constexpr (DELTA) lane_delta<E>(in, e0, w);
            to_planes<E>(w, pl);
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const uint64_t t0 = bit_tr8((uint64_t)pl[4 * j] | ((uint64_t)pl[4 * j + 1] << 32));      // elements 0 .. 7: byte k = bit plane 8 j + k
                const uint64_t t1 = bit_tr8((uint64_t)pl[4 * j + 2] | ((uint64_t)pl[4 * j + 3] << 32));  // elements 8 .. 15
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint32_t a = (uint32_t)(t0 >> (k < 4 ? 0 : 32)), b = (uint32_t)(t1 >> (k < 4 ? 0 : 32));
                    const uint32_t sel = 0x0C0C0000u | (uint32_t)(k & 3) | ((uint32_t)(4 + (k & 3)) << 8);
                    reinterpret_cast<uint16_t*>(lds + 128u * (8 * j + k))[lane] = (uint16_t)perm(b, a, sel);
                }
            }
        }
        wave_sync();
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const uint32_t p = 8u * j + (lane >> 3);
            const uint64_t c = t * 8u + (lane & 7u);
            if (c < C) store16(out + (uint64_t)p * nb + hq + 16u * c, *reinterpret_cast<const u32x4*>(lds + 128u * p + 16u * (lane & 7u)));
        }
        wave_sync();                                     // (the next tile writes the same slots)
        if (t == 0u) {
            bitshuffle_narrow<E, DELTA>(in, out, nb, 0u, hq, lane);
            bitshuffle_narrow<E, DELTA>(in, out, nb, hq + 16u * C, nb, lane);
            if constexpr (DELTA) delta_narrow<E>(in, out, nb * 8u, L / E, lane);
            copy_bytes(in, out, DELTA ? L / E * E : body, L, lane);
        }
    }
}

template <int E, bool DELTA>
__device__ __forceinline__ void unbitshuffle_block(const uint8_t* in, uint8_t* out, uint64_t L, uint64_t sub, uint64_t P, uint32_t lane, bool bytewise,
                                                   uint8_t* lds) {
    const uint64_t nb = L / E / 8u;
    const uint64_t body = nb * 8u * E;
    if constexpr (DELTA) {
        if (bytewise || ((uintptr_t)out & 15u) != 0u) {  // segments of all L / E elements: the residue behind m8 is summed with the rest
            const uint64_t m = L / E, nt = tiles_of(m, TILE);
            for (uint64_t t = sub; t < nt; t += P) {
                undelta_narrow_tile<FILTER_BITSHUFFLE, E>(in, out, m, t, 0u, lane);
                if (t == 0u) copy_bytes(in, out, m * E, L, lane);
            }
            return;
        }
    }
    if (bytewise || ((uintptr_t)out & 15u) != 0u) {      // a lane's 16 elements start a multiple of 16 E bytes behind `out`
        const uint64_t nt = tiles_of(nb, TILE / 8u);
        for (uint64_t t = sub; t < nt; t += P) {
            const uint64_t a = t * (TILE / 8u), b = a + TILE / 8u < nb ? a + TILE / 8u : nb;
            unbitshuffle_narrow<E>(in, out, nb, a, b, lane);
            if (t == 0u) copy_bytes(in, out, body, L, lane);
        }
        return;
    }
    const uint64_t C = nb / 16u;
    const uint64_t nt = tiles_of(C, 8u);
    for (uint64_t t = sub; t < nt; t += P) {
#pragma unroll
        for (int j = 0; j < E; ++j) {                    // every plane byte of the tile is read once
            const uint32_t p = 8u * j + (lane >> 3);
            const uint64_t c = t * 8u + (lane & 7u);
            if (c < C) *reinterpret_cast<u32x4*>(lds + 128u * p + 16u * (lane & 7u)) = load16(in + (uint64_t)p * nb + 16u * c);
        }
        wave_sync();
        const uint64_t g = t * 64u + lane;
        if ((g >> 3) < C) {
            uint32_t w[4 * E], pl[4 * E];
#pragma unroll
            for (int j = 0; j < E; ++j) {
                uint32_t a0 = 0u, a1 = 0u, b0 = 0u, b1 = 0u;         // t0 = a1:a0 (elements 0 .. 7), t1 = b1:b0
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint32_t u = reinterpret_cast<const uint16_t*>(lds + 128u * (8 * j + k))[lane];
                    const uint32_t lo = (u & 0xFFu) << (8 * (k & 3)), hi = (u >> 8) << (8 * (k & 3));
                    if (k < 4) { a0 |= lo; b0 |= hi; } else { a1 |= lo; b1 |= hi; }
                }
                const uint64_t x0 = bit_tr8((uint64_t)a0 | ((uint64_t)a1 << 32)), x1 = bit_tr8((uint64_t)b0 | ((uint64_t)b1 << 32));
                pl[4 * j] = (uint32_t)x0; pl[4 * j + 1] = (uint32_t)(x0 >> 32); pl[4 * j + 2] = (uint32_t)x1; pl[4 * j + 3] = (uint32_t)(x1 >> 32);
            }
            from_planes<E>(pl, w);
            if constexpr (DELTA) lz4flex_delta::carry16<E>(w, wave_exclusive_sum<E>(lz4flex_delta::scan16<E>(w), lane));      // (lane 0 starts a segment)
            const uint64_t e0 = g * LANE_ELEMS;
#pragma unroll
            for (int v = 0; v < E; ++v) store16(out + e0 * E + 16u * v, u32x4{w[4 * v], w[4 * v + 1], w[4 * v + 2], w[4 * v + 3]});
        }
        wave_sync();
        if (t == 0u) {
            if constexpr (DELTA) {
                undelta_narrow_from<FILTER_BITSHUFFLE, E>(in, out, L / E, 128u * C, lane);
                copy_bytes(in, out, L / E * E, L, lane);
            } else {
                unbitshuffle_narrow<E>(in, out, nb, 16u * C, nb, lane);
                copy_bytes(in, out, body, L, lane);
            }
        }
    }
}

__device__ __forceinline__ void copy_block(const uint8_t* in, uint8_t* out, uint64_t L, uint64_t sub, uint64_t P, uint32_t lane) {
    const uint64_t nt = (L + COPY_TILE - 1u) / COPY_TILE;
    for (uint64_t t = sub; t < nt; t += P) {
        const uint64_t a = t * COPY_TILE, len = L - a < COPY_TILE ? L - a : COPY_TILE;
        copy_range(out + a, in + a, len, lane, 64u);
    }
}

// FILTER_NONE | DELTA (and SHUFFLE | DELTA at E = 1), forward: d lies where x lay.  The wide path as unshuffle_block has it: elements that
// line up with 16-byte stores, h of them in front of the first aligned one.
template <int E>
__device__ __forceinline__ void delta_block(const uint8_t* in, uint8_t* out, uint64_t L, uint64_t sub, uint64_t P, uint32_t lane, bool bytewise) {
    const uint64_t m = L / E;
    if (bytewise || ((uintptr_t)out & (E - 1u)) != 0u) {
        const uint64_t nt = tiles_of(m, TILE);
        for (uint64_t t = sub; t < nt; t += P) {
            const uint64_t a = t * TILE, b = a + TILE < m ? a + TILE : m;
            delta_narrow<E>(in, out, a, b, lane);
            if (t == 0u) copy_bytes(in, out, m * E, L, lane);
        }
        return;
    }
    uint64_t h = ((16u - ((uintptr_t)out & 15u)) & 15u) / E;
    if (h > m) h = m;
    const uint64_t G = (m - h) / LANE_ELEMS;
    const uint64_t nt = tiles_of(G, 64u);
    for (uint64_t t = sub; t < nt; t += P) {
        const uint64_t g = t * 64u + lane;
        if (g < G) {
            const uint64_t e0 = h + g * LANE_ELEMS;
            uint32_t w[4 * E];
#pragma unroll
            for (int v = 0; v < E; ++v) {
                const u32x4 x = load16(in + e0 * E + 16u * v);
                w[4 * v] = x.x; w[4 * v + 1] = x.y; w[4 * v + 2] = x.z; w[4 * v + 3] = x.w;
            }
            lane_delta<E>(in, e0, w);
#pragma unroll
            for (int v = 0; v < E; ++v) store16(out + e0 * E + 16u * v, u32x4{w[4 * v], w[4 * v + 1], w[4 * v + 2], w[4 * v + 3]});
        }
        if (t == 0u) {
            delta_narrow<E>(in, out, 0u, h, lane);
            delta_narrow<E>(in, out, h + G * LANE_ELEMS, m, lane);
            copy_bytes(in, out, m * E, L, lane);
        }
    }
}

// its inverse: the wide path for an `out` that is 16-byte aligned (a tile starts on a restart), the narrow one for every other
template <int E>
__device__ __forceinline__ void undelta_block(const uint8_t* in, uint8_t* out, uint64_t L, uint64_t sub, uint64_t P, uint32_t lane, bool bytewise) {
    const uint64_t m = L / E;
    if (bytewise || ((uintptr_t)out & 15u) != 0u) {
        const uint64_t nt = tiles_of(m, TILE);
        for (uint64_t t = sub; t < nt; t += P) {
            undelta_narrow_tile<FILTER_NONE, E>(in, out, m, t, 0u, lane);
            if (t == 0u) copy_bytes(in, out, m * E, L, lane);
        }
        return;
    }
    const uint64_t G = m / LANE_ELEMS;
    const uint64_t nt = tiles_of(G, 64u);
    for (uint64_t t = sub; t < nt; t += P) {
        const uint64_t g = t * 64u + lane;
        if (g < G) {
            const uint64_t e0 = g * LANE_ELEMS;
            uint32_t w[4 * E];
#pragma unroll
            for (int v = 0; v < E; ++v) {
                const u32x4 x = load16(in + e0 * E + 16u * v);
                w[4 * v] = x.x; w[4 * v + 1] = x.y; w[4 * v + 2] = x.z; w[4 * v + 3] = x.w;
            }
            lz4flex_delta::carry16<E>(w, wave_exclusive_sum<E>(lz4flex_delta::scan16<E>(w), lane));
#pragma unroll
            for (int v = 0; v < E; ++v) store16(out + e0 * E + 16u * v, u32x4{w[4 * v], w[4 * v + 1], w[4 * v + 2], w[4 * v + 3]});
        }
        if (t == 0u) {
            undelta_narrow_from<FILTER_NONE, E>(in, out, m, G * LANE_ELEMS, lane);
            copy_bytes(in, out, m * E, L, lane);
        }
    }
}

template <int KIND, int E, bool DELTA>
__global__ void __launch_bounds__(THREADS) lz4_filter_kernel(FilterArgs a) {
    constexpr bool BITS = KIND == K_BITSHUFFLE || KIND == K_UNBITSHUFFLE;
    __shared__ __attribute__((aligned(16))) uint8_t lds[BITS ? WAVES * 1024u * E : 16u];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t W = (uint64_t)gridDim.x * WAVES, w = (uint64_t)blockIdx.x * WAVES + wv;
    const uint64_t P = W / a.n ? W / a.n : 1u;
    const uint64_t slots = (uint64_t)a.n * P;
    for (uint64_t s = w; s < slots; s += W) {
        const uint64_t b = s / P, sub = s % P;
        if (a.gate && a.gate[b] != 0) continue;
        const uint64_t L = a.len[b];
        const uint8_t* in = a.in_base + a.in_off[b];
        uint8_t* out = a.out_base + a.out_off[b];
        if constexpr (KIND == K_SHUFFLE) shuffle_block<E, DELTA>(in, out, L, sub, P, lane, a.bytewise != 0u);
        else if constexpr (KIND == K_UNSHUFFLE) unshuffle_block<E, DELTA>(in, out, L, sub, P, lane, a.bytewise != 0u);
        else if constexpr (KIND == K_BITSHUFFLE) bitshuffle_block<E, DELTA>(in, out, L, sub, P, lane, a.bytewise != 0u, lds + wv * 1024u * E);
        else if constexpr (KIND == K_UNBITSHUFFLE) unbitshuffle_block<E, DELTA>(in, out, L, sub, P, lane, a.bytewise != 0u, lds + wv * 1024u * E);
        else if constexpr (KIND == K_DELTA) delta_block<E>(in, out, L, sub, P, lane, a.bytewise != 0u);
        else if constexpr (KIND == K_UNDELTA) undelta_block<E>(in, out, L, sub, P, lane, a.bytewise != 0u);
        else copy_block(in, out, L, sub, P, lane);
    }
}

template <int KIND, int E, bool DELTA = false>
hipError_t launch_one(const FilterArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((lz4_filter_kernel<KIND, E, DELTA>), dim3(GRID), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}
template <int KIND, bool DELTA = false>
hipError_t launch_elem(const FilterArgs& a, uint32_t elem, hipStream_t s) {
    switch (elem) {
        case 1u: return launch_one<KIND, 1, DELTA>(a, s);
        case 2u: return launch_one<KIND, 2, DELTA>(a, s);
        case 4u: return launch_one<KIND, 4, DELTA>(a, s);
        case 8u: return launch_one<KIND, 8, DELTA>(a, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_filter(const FilterArgs& a, int filter, uint32_t elem, bool inverse, hipStream_t s) {
    if (a.n == 0u) return hipSuccess;
    if (elem != 1u && elem != 2u && elem != 4u && elem != 8u) return hipErrorInvalidValue;
    if ((filter & ~FILTER_DELTA) != FILTER_NONE && (filter & ~FILTER_DELTA) != FILTER_SHUFFLE && (filter & ~FILTER_DELTA) != FILTER_BITSHUFFLE) return hipErrorInvalidValue;
    if (filter & FILTER_DELTA) {                         // one launch as well: the delta stage runs in the base filter's lanes
        const int base = filter & ~FILTER_DELTA;
        if (base == FILTER_NONE || (base == FILTER_SHUFFLE && elem == 1u)) return inverse ? launch_elem<K_UNDELTA, true>(a, elem, s) : launch_elem<K_DELTA, true>(a, elem, s);
        if (base == FILTER_SHUFFLE) return inverse ? launch_elem<K_UNSHUFFLE, true>(a, elem, s) : launch_elem<K_SHUFFLE, true>(a, elem, s);
        return inverse ? launch_elem<K_UNBITSHUFFLE, true>(a, elem, s) : launch_elem<K_BITSHUFFLE, true>(a, elem, s);
    }
    if (filter == FILTER_NONE || (filter == FILTER_SHUFFLE && elem == 1u)) return launch_one<K_COPY, 1>(a, s);
    if (filter == FILTER_SHUFFLE) return inverse ? launch_elem<K_UNSHUFFLE>(a, elem, s) : launch_elem<K_SHUFFLE>(a, elem, s);
    if (filter == FILTER_BITSHUFFLE) return inverse ? launch_elem<K_UNBITSHUFFLE>(a, elem, s) : launch_elem<K_BITSHUFFLE>(a, elem, s);
    return hipErrorInvalidValue;
}

}  // namespace lz4flex_dev
