// frame_range.hip -- the device side of a frame index and of range reads through it (frame_index.cpp).
//
// What it replaces: nothing in the reference -- a FrameDecoder (src/frame/decompress.rs:189-342) reads a frame from its first byte on.
// Here a frame that is structurally sound gets a block table once (index kernels), and a call that wants byte ranges of the content
// turns each range into work on the blocks it touches (plan kernel), runs the existing batch launches over that work, and folds the
// per-block results into one verdict per range (verdict kernel).  The decoders, the scans and the walk are launched as they are.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lz4flex_amd.h"
#include "frame_range.h"
#include "lz4_device.h"

namespace lz4flex_dev {

using lz4flex_range::RangeRec;

// ---- the index ---------------------------------------------------------------------------------------------------------------------
// block b of the walk's table: the length the size scan sees -- a stored block is not scanned (length 0: its status is not read)
__global__ void __launch_bounds__(256) frame_index_prep_kernel(const uint32_t* __restrict__ word, uint32_t n, uint32_t* __restrict__ scan_len,
                                                               uint32_t* __restrict__ first_bad) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0u) { first_bad[0] = 0xFFFFFFFFu; first_bad[1] = 0xFFFFFFFFu; }
    if (b >= n) return;
    const uint32_t w = word[b];
    scan_len[b] = (w & 0x80000000u) ? 0u : w;
}

// size[b] = the block's decoded bytes: a stored block's length, a compressed block's scanned size; first_bad[0] = the first compressed
// block that does not scan or decodes to more than the frame's block size (its size counts as 0), first_bad[1] = the first sound block
// of no bytes at all (there a reader's read_to_end ends, src/frame/decompress.rs:344-349)
__global__ void __launch_bounds__(256) frame_index_sizes_kernel(const uint32_t* __restrict__ word, const int32_t* __restrict__ scan_st, uint32_t n,
                                                                uint32_t block_size, uint64_t* __restrict__ size, uint32_t* __restrict__ first_bad) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    const uint32_t w = word[b];
    if (w & 0x80000000u) {
        size[b] = w & 0x7FFFFFFFu;
        if ((w & 0x7FFFFFFFu) == 0u) atomicMin(first_bad + 1, b);
        return;
    }
    if (scan_st[b] != 0 || size[b] > block_size) { size[b] = 0ull; atomicMin(first_bad, b); }
    else if (size[b] == 0ull) atomicMin(first_bad + 1, b);
}

hipError_t launch_frame_index_prep(const uint32_t* word, uint32_t n, uint32_t* scan_len, uint32_t* first_bad, hipStream_t s) {
    hipLaunchKernelGGL(frame_index_prep_kernel, dim3(n ? (n + 255u) / 256u : 1u), dim3(256), 0, s, word, n, scan_len, first_bad);
    return hipGetLastError();
}
hipError_t launch_frame_index_sizes(const uint32_t* word, const int32_t* scan_st, uint32_t n, uint32_t block_size, uint64_t* size, uint32_t* first_bad,
                                    hipStream_t s) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(frame_index_sizes_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, word, scan_st, n, block_size, size, first_bad);
    return hipGetLastError();
}

// ---- a pass of range reads ---------------------------------------------------------------------------------------------------------
// the range item slot t belongs to: the LAST r with rec[r].slot <= t (ranges without blocks share their slot with the range behind them)
__device__ __forceinline__ uint32_t range_of_slot(const RangeRec* __restrict__ rec, uint32_t n_ranges, uint32_t t) {
    uint32_t lo = 0u, hi = n_ranges;                  // rec[lo].slot <= t; hi == n_ranges or rec[hi].slot > t
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (rec[mid].slot <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// One thread per touched block (t < n_slots) writes that block's descriptors; thread r < n_ranges writes range r's scratch items when
// the range has no head (a head's thread -- the range's first slot -- writes them otherwise).
//   decode batch A (sink: the output): a compressed block that is not a head, from its first byte up to the range's end in it
//   decode batch B (sink: scratch):    a head, up to its last wanted byte
//   copies from the input:             a stored block's wanted span
//   copies from scratch:               a head's wanted span
//   checksums:                         every touched payload, whole
__global__ void __launch_bounds__(256) frame_range_plan_kernel(FrameRangePlan p) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < p.n_ranges && p.rec[t].head == 0u) {
        p.b_in[t] = 0ull; p.b_len[t] = 0u; p.b_out[t] = 0ull; p.b_tgt[t] = 0u;
        p.d_src[t] = 0ull; p.d_len[t] = 0u; p.d_dst[t] = 0ull;
    }
    if (t >= p.n_slots) return;
    const uint32_t r = range_of_slot(p.rec, p.n_ranges, t);
    const RangeRec q = p.rec[r];
    const uint32_t b = q.b0 + (t - q.slot);
    const uint64_t c0 = p.content_off[b], c1 = p.content_off[b + 1u];
    const uint32_t w = p.len_word[b], plen = w & 0x7FFFFFFFu;
    const bool stored = (w & 0x80000000u) != 0u;
    const uint64_t pay = (uint64_t)((int64_t)p.payload_off[b] + q.shift);
    const uint64_t end = q.off + q.len;
    const uint64_t lo = q.off > c0 ? q.off : c0, hi = end < c1 ? end : c1;       // the wanted bytes of this block: [lo, hi), lo <= hi
    const uint64_t dst = q.out_off + (lo - q.off);
    const bool head = q.head != 0u && t == q.slot;
    p.a_in[t] = pay; p.a_len[t] = plen; p.a_out[t] = dst;
    p.a_tgt[t] = (stored || head) ? 0u : (uint32_t)(hi - c0);
    p.c_src[t] = pay + (stored ? lo - c0 : 0ull); p.c_len[t] = stored ? (uint32_t)(hi - lo) : 0u; p.c_dst[t] = dst;
    if (head) {
        p.b_in[r] = pay; p.b_len[r] = plen; p.b_out[r] = q.head_off; p.b_tgt[r] = (uint32_t)(hi - c0);
        p.d_src[r] = q.head_off + (lo - c0); p.d_len[r] = (uint32_t)(hi - lo); p.d_dst[r] = q.out_off;
    }
}

hipError_t launch_frame_range_plan(const FrameRangePlan& p, hipStream_t s) {
    const uint32_t n = p.n_slots > p.n_ranges ? p.n_slots : p.n_ranges;
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(frame_range_plan_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, p);
    return hipGetLastError();
}

// One wavefront per range: the first touched block, in stream order, that is defective decides -- its checksum before its decode
// (src/frame/decompress.rs:255-261 before :280-306).  A compressed block that decodes without an error but to fewer bytes than the
// index says (the frame changed since the index was made) is a decode defect with inner 0 and expected / actual = wanted / produced.
__global__ void __launch_bounds__(64) frame_range_verdict_kernel(FrameRangeVerdict v) {
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    if (r >= v.n_ranges) return;
    const RangeRec q = v.rec[r];
    uint32_t bad_j = 0xFFFFFFFFu;
    int32_t code = 0, inner = 0;
    uint64_t want = 0ull, got = 0ull;
    for (uint32_t j = lane; j < q.nb; j += 64u) {
        const uint32_t t = q.slot + j;
        if (v.bad != nullptr && v.bad[t] != 0u) { bad_j = j; code = -LZ4FLEX_FE_BLOCK_CHECKSUM; break; }
        if (v.len_word[q.b0 + j] & 0x80000000u) continue;
        const bool head = q.head != 0u && j == 0u;
        const int32_t st = head ? v.b_st[r] : v.a_st[t];
        const uint32_t tgt = head ? v.b_tgt[r] : v.a_tgt[t], len = head ? v.b_olen[r] : v.a_olen[t];
        if (st != 0 || len != tgt) {
            bad_j = j; code = -LZ4FLEX_FE_DECOMPRESSION; inner = st;
            if (st == 0) { want = tgt; got = len; }
            break;
        }
    }
    uint32_t first = bad_j;
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)first, d, 64);
        first = o < first ? o : first;
    }
    if (first == 0xFFFFFFFFu) {
        if (lane == 0u) { v.status[r] = 0; v.out_len[r] = q.len; v.inner[r] = 0; v.expected[r] = 0ull; v.actual[r] = 0ull; }
    } else if (bad_j == first) {
        v.status[r] = code; v.out_len[r] = 0ull; v.inner[r] = inner; v.expected[r] = want; v.actual[r] = got;
    }
}

hipError_t launch_frame_range_verdict(const FrameRangeVerdict& v, hipStream_t s) {
    if (v.n_ranges == 0u) return hipSuccess;
    hipLaunchKernelGGL(frame_range_verdict_kernel, dim3(v.n_ranges), dim3(64), 0, s, v);
    return hipGetLastError();
}

}  // namespace lz4flex_dev
