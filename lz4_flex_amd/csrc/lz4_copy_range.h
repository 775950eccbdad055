// lz4_copy_range.h -- the byte-range copy of a workgroup that the kernels which lay produced bytes out back to back share
// (frame_kernels.hip: frame segments, lz4_packed.hip: packed blocks).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4_wave_prims.h"

namespace lz4flex_dev {

// thread t of nt copies its share of src[0, n) to dst: 16 bytes per lane where source and destination allow it
__device__ __forceinline__ void copy_range(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint64_t n, uint32_t t, uint32_t nt) {
    if ((((uintptr_t)dst | (uintptr_t)src) & 15u) == 0u) {
        const uint64_t nv = n / 16u;
        for (uint64_t i = t; i < nv; i += nt) reinterpret_cast<u32x4*>(dst)[i] = reinterpret_cast<const u32x4*>(src)[i];
        for (uint64_t i = nv * 16u + t; i < n; i += nt) dst[i] = src[i];
    } else if (((uintptr_t)dst & 15u) == ((uintptr_t)src & 15u)) {
        const uint64_t head = (16u - ((uintptr_t)dst & 15u)) & 15u;
        const uint64_t h = head < n ? head : n;
        for (uint64_t i = t; i < h; i += nt) dst[i] = src[i];
        const uint64_t nv = (n - h) / 16u;
        for (uint64_t i = t; i < nv; i += nt) reinterpret_cast<u32x4*>(dst + h)[i] = reinterpret_cast<const u32x4*>(src + h)[i];
        for (uint64_t i = h + nv * 16u + t; i < n; i += nt) dst[i] = src[i];
    } else {
        // different phase: aligned 16-byte stores, unaligned loads (global memory takes any alignment)
        const uint64_t head = (16u - ((uintptr_t)dst & 15u)) & 15u;
        const uint64_t h = head < n ? head : n;
        for (uint64_t i = t; i < h; i += nt) dst[i] = src[i];
        const uint64_t nv = (n - h) / 16u;
        for (uint64_t i = t; i < nv; i += nt) {
            u32x4 v;
            __builtin_memcpy(&v, src + h + 16u * i, 16);
            reinterpret_cast<u32x4*>(dst + h)[i] = v;
        }
        for (uint64_t i = h + nv * 16u + t; i < n; i += nt) dst[i] = src[i];
    }
}

}  // namespace lz4flex_dev
