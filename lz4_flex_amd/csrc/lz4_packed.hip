// lz4_packed.hip -- the layout kernels of the packed batch entries (lz4flex_decompress_batch_packed, lz4flex_compress_batch_packed):
// the caller hands over blocks and ONE output buffer, the offsets are computed here, on the device, in front of (decode) or behind
// (compress) the codec's own launch.
//   packed_sizes_kernel        the slot size of every block as a u64: the LE u32 prefix of a size-prepended block (block::uncompressed_size,
//                              src/block/mod.rs:151-157), the caller's capacity, what the size scan measured; compress side:
//                              get_maximum_output_size for the scratch slots, later the produced lengths for the packed stream;
//   packed_tile_sums_kernel,   an exclusive scan of the sizes, each rounded up to `align`, over any n, in three phases: every workgroup
//   packed_tile_scan_kernel,   sums its tile of PACKED_SCAN_TILE sizes, ONE workgroup scans the tile sums (any number of them: a thread
//   packed_offsets_kernel      takes a contiguous share), every workgroup scans its tile from its tile's base.  Integer sums in a fixed
//                              order: the result does not depend on how the workgroups are scheduled.  The last phase applies the FIT
//                              RULE: block i fits iff off[i] + size[i] <= total_cap; a block that does not fit gets capacity 0;
//   packed_finish_kernel       decode: the blocks that were not handed to the decoder as they are (no size, no room) get their status,
//                              and every block that is not OutputTooSmall the detail {0, 0};
//   packed_gather_kernel       compress: scratch slot -> out_base + off[i], a workgroup per block, with the LE u32 length prefix.
// Every store is a plain vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4_copy_range.h"
#include "lz4_device.h"

namespace lz4flex_dev {

namespace {

constexpr uint32_t THREADS = 256u;
constexpr uint32_t PER_THREAD = PACKED_SCAN_TILE / THREADS;
static_assert(PER_THREAD * THREADS == PACKED_SCAN_TILE, "a tile is a whole number of elements per thread");
constexpr uint32_t MAX_GRID = 1u << 22;                 // workgroups per launch; the kernels stride over what is left

__device__ __forceinline__ uint64_t round_up(uint64_t v, uint32_t align) { return (v + (align - 1u)) & ~(uint64_t)(align - 1u); }

// inclusive scan of one value per thread across the workgroup (Hillis-Steele over LDS); returns this thread's inclusive sum
__device__ __forceinline__ uint64_t workgroup_scan(uint64_t v, uint64_t* part) {
    const uint32_t t = threadIdx.x;
    part[t] = v;
    __syncthreads();
    for (uint32_t d = 1u; d < THREADS; d <<= 1) {
        const uint64_t u = t >= d ? part[t - d] : 0ull;
        __syncthreads();
        part[t] += u;
        __syncthreads();
    }
    const uint64_t r = part[t];
    __syncthreads();                                     // (the caller may scan again)
    return r;
}

}  // namespace

__global__ void __launch_bounds__(256) packed_sizes_kernel(int mode, const uint8_t* __restrict__ in_base, const uint64_t* __restrict__ in_off,
                                                           const uint32_t* __restrict__ in_len, const uint32_t* __restrict__ given,
                                                           const int32_t* __restrict__ given_st, uint32_t n, uint32_t extra,
                                                           uint64_t* __restrict__ size, uint64_t* __restrict__ sh_off,
                                                           uint32_t* __restrict__ sh_len, int32_t* __restrict__ pre) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        if (mode == PACKED_SIZES_PREPENDED) {
            const uint32_t len = in_len[i];
            const uint64_t at = in_off[i];
            if (len < 4u) {                                                    // mod.rs:152
                size[i] = 0ull; sh_off[i] = at; sh_len[i] = 0u; pre[i] = LZ4FLEX_DEV_E_EXPECTED_ANOTHER_BYTE;
            } else {
                const uint8_t* p = in_base + at;                               // (any alignment is legal: byte by byte)
                size[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
                sh_off[i] = at + 4ull; sh_len[i] = len - 4u; pre[i] = 0;
            }
        } else if (mode == PACKED_SIZES_GIVEN) {
            size[i] = given[i]; pre[i] = 0;
        } else if (mode == PACKED_SIZES_SCAN) {                                // size / pre hold the size pass's results
            if (pre[i] != 0) size[i] = 0ull;
            else if (size[i] > 0xFFFFFFFFull) { size[i] = 0ull; pre[i] = LZ4FLEX_DEV_E_UNSUPPORTED; }   // the decoders' out_cap is a u32
        } else if (mode == PACKED_SIZES_SLOTS) {                               // get_maximum_output_size, compress.rs:588-590
            size[i] = 20ull + (uint64_t)in_len[i] * 110ull / 100ull + extra; pre[i] = 0;
        } else {                                                               // PACKED_SIZES_PRODUCED: what the encoder wrote
            size[i] = given_st[i] == 0 ? (uint64_t)given[i] + extra : 0ull;
        }
    }
}

__global__ void __launch_bounds__(256) packed_tile_sums_kernel(const uint64_t* __restrict__ size, uint32_t n, uint32_t align,
                                                               uint32_t n_tiles, uint64_t* __restrict__ tiles) {
    __shared__ uint64_t part[THREADS];
    const uint32_t t = threadIdx.x;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t base = (uint64_t)tile * PACKED_SCAN_TILE;
        uint64_t s = 0ull;
        for (uint32_t k = 0; k < PER_THREAD; ++k) {
            const uint64_t i = base + (uint64_t)k * THREADS + t;
            if (i < n) s += round_up(size[i], align);
        }
        part[t] = s;
        __syncthreads();
        for (uint32_t d = THREADS / 2u; d != 0u; d >>= 1) {
            if (t < d) part[t] += part[t + d];
            __syncthreads();
        }
        if (t == 0u) tiles[tile] = part[0];
        __syncthreads();
    }
}

// ONE workgroup: tiles[0 .. n_tiles) become their exclusive sums, *total the sum of all
__global__ void __launch_bounds__(256) packed_tile_scan_kernel(uint64_t* __restrict__ tiles, uint32_t n_tiles, uint64_t* __restrict__ total) {
    __shared__ uint64_t part[THREADS];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n_tiles + THREADS - 1u) / THREADS;
    const uint64_t lo = (uint64_t)t * per, hi = lo + per < n_tiles ? lo + per : n_tiles;
    uint64_t s = 0ull;
    for (uint64_t i = lo; i < hi; ++i) s += tiles[i];
    const uint64_t incl = workgroup_scan(s, part);
    uint64_t o = incl - s;
    for (uint64_t i = lo; i < hi; ++i) { const uint64_t v = tiles[i]; tiles[i] = o; o += v; }
    if (t == THREADS - 1u) *total = incl;
}

__global__ void __launch_bounds__(256) packed_offsets_kernel(const uint64_t* __restrict__ size, const uint64_t* __restrict__ tiles, uint32_t n,
                                                             uint32_t n_tiles, uint32_t align, uint64_t total_cap, uint32_t shift,
                                                             uint64_t* __restrict__ off, uint64_t* __restrict__ place,
                                                             uint32_t* __restrict__ cap, int32_t* __restrict__ pre) {
    __shared__ uint64_t part[THREADS];
    const uint32_t t = threadIdx.x;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t first = (uint64_t)tile * PACKED_SCAN_TILE + (uint64_t)t * PER_THREAD;
        uint64_t sz[PER_THREAD];
        uint64_t s = 0ull;
        for (uint32_t k = 0; k < PER_THREAD; ++k) {
            sz[k] = first + k < n ? size[first + k] : 0ull;
            s += first + k < n ? round_up(sz[k], align) : 0ull;
        }
        uint64_t o = tiles[tile] + workgroup_scan(s, part) - s;
        for (uint32_t k = 0; k < PER_THREAD; ++k) {
            const uint64_t i = first + k;
            if (i >= n) break;
            const bool fits = o + sz[k] <= total_cap;
            off[i] = o;
            if (place) place[i] = fits ? o + shift : 0ull;
            if (cap) { const uint64_t c = sz[k] - shift; cap[i] = fits ? (uint32_t)(c > 0xFFFFFFFFull ? 0xFFFFFFFFull : c) : 0u; }
            if (pre && !fits) pre[i] = LZ4FLEX_DEV_E_OUTPUT_TOO_SMALL;
            o += round_up(sz[k], align);
        }
    }
}

__global__ void __launch_bounds__(256) packed_finish_kernel(const int32_t* __restrict__ pre, const uint64_t* __restrict__ size,
                                                            const uint64_t* __restrict__ off, uint32_t n, uint64_t total_cap,
                                                            uint32_t* __restrict__ out_len, int32_t* __restrict__ status,
                                                            uint64_t* __restrict__ detail) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const int32_t p = pre[i];
        if (p != 0) { status[i] = p; out_len[i] = 0u; }
        if (detail) {
            // the decoders fill the detail of an OutputTooSmall block only: every other block gets {0, 0} here
            const bool room = p == LZ4FLEX_DEV_E_OUTPUT_TOO_SMALL;             // (as pre[], only the fit rule gives this one)
            if (room) { detail[2u * i] = off[i] + size[i]; detail[2u * i + 1u] = total_cap; }
            else if (p != 0 || status[i] != LZ4FLEX_DEV_E_OUTPUT_TOO_SMALL) { detail[2u * i] = 0ull; detail[2u * i + 1u] = 0ull; }
        }
    }
}

__global__ void __launch_bounds__(256) packed_gather_kernel(const uint8_t* __restrict__ scratch, const uint64_t* __restrict__ src_off,
                                                            const uint64_t* __restrict__ size, const uint64_t* __restrict__ off,
                                                            const uint32_t* __restrict__ in_len, uint32_t n, uint32_t prefix,
                                                            uint64_t total_cap, uint8_t* __restrict__ out, uint32_t* __restrict__ out_len,
                                                            int32_t* __restrict__ status) {
    for (uint32_t b = blockIdx.x; b < n; b += gridDim.x) {
        const uint64_t sz = size[b], o = off[b];
        const bool fits = o + sz <= total_cap;
        const bool ok = status[b] == 0;
        __syncthreads();                                                       // (every lane has read the status before lane 0 writes it)
        if (!ok || !fits) {
            if (threadIdx.x == 0u) { out_len[b] = 0u; if (!fits) status[b] = LZ4FLEX_DEV_E_OUTPUT_TOO_SMALL; }
            continue;
        }
        uint8_t* d = out + o;
        if (threadIdx.x == 0u) {
            out_len[b] = (uint32_t)sz;
            if (prefix) { const uint32_t w = in_len[b]; d[0] = (uint8_t)w; d[1] = (uint8_t)(w >> 8); d[2] = (uint8_t)(w >> 16); d[3] = (uint8_t)(w >> 24); }
        }
        copy_range(d + prefix, scratch + src_off[b], sz - prefix, threadIdx.x, THREADS);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static inline uint32_t tiles_of(uint32_t n) { return (uint32_t)(((uint64_t)n + PACKED_SCAN_TILE - 1u) / PACKED_SCAN_TILE); }

size_t packed_work_bytes(uint32_t n) {
    const size_t m = n;
    return up256(8u * m) + up256(8u * m) + up256(8u * (m + 1u)) + up256(8u * ((size_t)tiles_of(n) + 1u)) + up256(4u * m) + up256(4u * m);
}

PackedWork packed_work(void* work, uint32_t n) {
    const size_t m = n;
    uint8_t* p = (uint8_t*)work;
    PackedWork w;
    w.size = (uint64_t*)p; p += up256(8u * m);
    w.place = (uint64_t*)p; p += up256(8u * m);
    w.aux_off = (uint64_t*)p; p += up256(8u * (m + 1u));
    w.tiles = (uint64_t*)p; p += up256(8u * ((size_t)tiles_of(n) + 1u));
    w.aux_len = (uint32_t*)p; p += up256(4u * m);
    w.pre = (int32_t*)p;
    return w;
}

hipError_t launch_packed_sizes(int mode, const uint8_t* in_base, const uint64_t* in_off, const uint32_t* in_len, const uint32_t* given,
                               const int32_t* given_st, uint32_t n, uint32_t extra, uint64_t* size, uint64_t* sh_off, uint32_t* sh_len,
                               int32_t* pre, hipStream_t s) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(packed_sizes_kernel, dim3(grid_of(((uint64_t)n + THREADS - 1u) / THREADS)), dim3(THREADS), 0, s, mode, in_base, in_off,
                       in_len, given, given_st, n, extra, size, sh_off, sh_len, pre);
    return hipGetLastError();
}

hipError_t launch_packed_scan(const uint64_t* size, uint32_t n, uint32_t align, uint64_t total_cap, uint32_t shift, uint64_t* tiles,
                              uint64_t* off, uint64_t* place, uint32_t* cap, int32_t* pre, hipStream_t s) {
    if (n == 0u) return hipMemsetAsync(off, 0, 8, s);
    const uint32_t m = tiles_of(n);
    hipLaunchKernelGGL(packed_tile_sums_kernel, dim3(grid_of(m)), dim3(THREADS), 0, s, size, n, align, m, tiles);
    hipLaunchKernelGGL(packed_tile_scan_kernel, dim3(1), dim3(THREADS), 0, s, tiles, m, off + n);
    hipLaunchKernelGGL(packed_offsets_kernel, dim3(grid_of(m)), dim3(THREADS), 0, s, size, (const uint64_t*)tiles, n, m, align, total_cap,
                       shift, off, place, cap, pre);
    return hipGetLastError();
}

hipError_t launch_packed_finish(const int32_t* pre, const uint64_t* size, const uint64_t* off, uint32_t n, uint64_t total_cap,
                                uint32_t* out_len, int32_t* status, uint64_t* detail, hipStream_t s) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(packed_finish_kernel, dim3(grid_of(((uint64_t)n + THREADS - 1u) / THREADS)), dim3(THREADS), 0, s, pre, size, off, n,
                       total_cap, out_len, status, detail);
    return hipGetLastError();
}

hipError_t launch_packed_gather(const uint8_t* scratch, const uint64_t* src_off, const uint64_t* size, const uint64_t* off,
                                const uint32_t* in_len, uint32_t n, uint32_t prefix, uint64_t total_cap, uint8_t* out, uint32_t* out_len,
                                int32_t* status, hipStream_t s) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(packed_gather_kernel, dim3(grid_of(n)), dim3(THREADS), 0, s, scratch, src_off, size, off, in_len, n, prefix, total_cap,
                       out, out_len, status);
    return hipGetLastError();
}

}  // namespace lz4flex_dev
