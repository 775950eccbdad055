// lz4_wave_prims.h -- what the wavefront kernels share: the address-space and vector types and a few whole-wavefront (wave64)
// operations.  Device code only -- the headers that also compile as host simulations (-DLZ4FLEX_HOST_SIM) keep their own types.
// Only what more than one kernel file uses with the same meaning is here; an operation with one owner stays with its owner.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lz4flex_dev {

// a generic pointer would make every access a FLAT instruction; a pointer that crosses a call is flat unless its type names the space
typedef __attribute__((address_space(3))) uint8_t lds_u8;
typedef __attribute__((address_space(1))) uint8_t g_u8;
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// v from the lane the DPP control names, 0 where it names none (rmask: the rows that take part)
#define LZ4_DPP(v, ctrl, rmask) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), (ctrl), (rmask), 0xf, false))
// inclusive prefix sum over the 64 lanes
__device__ __forceinline__ uint32_t wave_incl_add(uint32_t v) {
    v += LZ4_DPP(v, 0x111, 0xf);     // row_shr:1
    v += LZ4_DPP(v, 0x112, 0xf);     // row_shr:2
    v += LZ4_DPP(v, 0x114, 0xf);     // row_shr:4
    v += LZ4_DPP(v, 0x118, 0xf);     // row_shr:8
    v += LZ4_DPP(v, 0x142, 0xa);     // row_bcast:15 -> rows 1, 3
    v += LZ4_DPP(v, 0x143, 0xc);     // row_bcast:31 -> rows 2, 3
    return v;
}
__device__ __forceinline__ uint32_t rdlane(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t ctz64(uint64_t x) { return (uint32_t)__builtin_ctzll(x); }

}  // namespace lz4flex_dev
