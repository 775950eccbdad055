// lz4_filter_delta.h -- the lane-local arithmetic of the delta stage of typed batches (LZ4FLEX_FILTER_DELTA; the definition:
// include/lz4flex_amd.h "typed batches"; the kernels: lz4_filter.hip).  A lane holds 16 consecutive elements of E bytes, little-endian, in
// 4 E dwords w[]: element i is byte i (E = 1), half i & 1 of w[i / 2] (E = 2), w[i] (E = 4), w[2 i + 1] : w[2 i] (E = 8).
//   delta16   forward:  d[i] = x[i] - x[i - 1] mod 2^(8 E), x[-1] = prev, and d[ri] = x[ri] for the one element ri (0 .. 15; 16 = none)
//             that starts a restart segment
//   scan16    inverse:  x[i] = d[0] + ... + d[i] mod 2^(8 E) in place; returns x[15], the lane's total
//   carry16   inverse:  x[i] += carry -- the sum of the lanes in front, from the wavefront scan
// E = 1 and E = 2 add and subtract 4 bytes / 2 halves per dword without a carry between them (SWAR: the top bit of every field goes by
// XOR), E = 8 is 64-bit arithmetic, which the compiler makes an add with carry over the two dwords.  Every index is a constant once
// unrolled, so w[] stays in registers.  Plain functions of their arguments: a host build (tests/sim/filter_delta_shim.cpp) compiles them
// as they are.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LZ4FLEX_DELTA_FN __host__ __device__ __forceinline__
#else
#define LZ4FLEX_DELTA_FN inline
#endif

namespace lz4flex_delta {

constexpr uint32_t RESTART = 1024u;                      // the header's LZ4FLEX_DELTA_RESTART

LZ4FLEX_DELTA_FN uint32_t add8(uint32_t a, uint32_t b) { return ((a & 0x7F7F7F7Fu) + (b & 0x7F7F7F7Fu)) ^ ((a ^ b) & 0x80808080u); }
LZ4FLEX_DELTA_FN uint32_t sub8(uint32_t a, uint32_t b) { return ((a | 0x80808080u) - (b & 0x7F7F7F7Fu)) ^ ((a ^ ~b) & 0x80808080u); }
LZ4FLEX_DELTA_FN uint32_t add16(uint32_t a, uint32_t b) { return ((a & 0x7FFF7FFFu) + (b & 0x7FFF7FFFu)) ^ ((a ^ b) & 0x80008000u); }
LZ4FLEX_DELTA_FN uint32_t sub16(uint32_t a, uint32_t b) { return ((a | 0x80008000u) - (b & 0x7FFF7FFFu)) ^ ((a ^ ~b) & 0x80008000u); }

template <int E>
LZ4FLEX_DELTA_FN void delta16(uint32_t* w, uint64_t prev, uint32_t ri) {
    if constexpr (E == 1) {
#pragma unroll
        for (int k = 3; k >= 0; --k) {                   // downwards: w[k - 1] is still x
            uint32_t p = (w[k] << 8) | (k ? w[k > 0 ? k - 1 : 0] >> 24 : (uint32_t)prev & 0xFFu);
            if ((ri >> 2) == (uint32_t)k) p &= ~(0xFFu << (8u * (ri & 3u)));
            w[k] = sub8(w[k], p);
        }
    } else if constexpr (E == 2) {
#pragma unroll
        for (int k = 7; k >= 0; --k) {
            uint32_t p = (w[k] << 16) | (k ? w[k > 0 ? k - 1 : 0] >> 16 : (uint32_t)prev & 0xFFFFu);
            if ((ri >> 1) == (uint32_t)k) p &= ~(0xFFFFu << (16u * (ri & 1u)));
            w[k] = sub16(w[k], p);
        }
    } else if constexpr (E == 4) {
#pragma unroll
        for (int k = 15; k >= 0; --k) {
            const uint32_t p = k ? w[k > 0 ? k - 1 : 0] : (uint32_t)prev;
            w[k] -= ri == (uint32_t)k ? 0u : p;
        }
    } else {
#pragma unroll
        for (int k = 15; k >= 0; --k) {
            const uint64_t x = (uint64_t)w[2 * k] | ((uint64_t)w[2 * k + 1] << 32);
            const uint64_t p = k ? (uint64_t)w[k > 0 ? 2 * k - 2 : 0] | ((uint64_t)w[k > 0 ? 2 * k - 1 : 1] << 32) : prev;
            const uint64_t d = x - (ri == (uint32_t)k ? 0ull : p);
            w[2 * k] = (uint32_t)d;
            w[2 * k + 1] = (uint32_t)(d >> 32);
        }
    }
}

template <int E>
LZ4FLEX_DELTA_FN uint64_t scan16(uint32_t* w) {
    if constexpr (E == 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t x = w[k];
            x = add8(x, x << 8);
            x = add8(x, x << 16);
            if (k) x = add8(x, (w[k > 0 ? k - 1 : 0] >> 24) * 0x01010101u);
            w[k] = x;
        }
        return w[3] >> 24;
    } else if constexpr (E == 2) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            uint32_t x = w[k];
            x = add16(x, x << 16);
            if (k) x = add16(x, (w[k > 0 ? k - 1 : 0] >> 16) * 0x00010001u);
            w[k] = x;
        }
        return w[7] >> 16;
    } else if constexpr (E == 4) {
#pragma unroll
        for (int k = 1; k < 16; ++k) w[k] += w[k - 1];
        return w[15];
    } else {
        uint64_t run = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            run += (uint64_t)w[2 * k] | ((uint64_t)w[2 * k + 1] << 32);
            w[2 * k] = (uint32_t)run;
            w[2 * k + 1] = (uint32_t)(run >> 32);
        }
        return run;
    }
}

template <int E>
LZ4FLEX_DELTA_FN void carry16(uint32_t* w, uint64_t carry) {
    if constexpr (E == 1) {
        const uint32_t c = ((uint32_t)carry & 0xFFu) * 0x01010101u;
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = add8(w[k], c);
    } else if constexpr (E == 2) {
        const uint32_t c = ((uint32_t)carry & 0xFFFFu) * 0x00010001u;
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = add16(w[k], c);
    } else if constexpr (E == 4) {
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k] += (uint32_t)carry;
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint64_t x = ((uint64_t)w[2 * k] | ((uint64_t)w[2 * k + 1] << 32)) + carry;
            w[2 * k] = (uint32_t)x;
            w[2 * k + 1] = (uint32_t)(x >> 32);
        }
    }
}

// the restart element among the 16 that start at element e0 of the block: its index, or 16
LZ4FLEX_DELTA_FN uint32_t restart_index(uint64_t e0) {
    const uint32_t r = (uint32_t)e0 & (RESTART - 1u);
    const uint32_t ri = r ? RESTART - r : 0u;
    return ri < 16u ? ri : 16u;
}

}  // namespace lz4flex_delta
