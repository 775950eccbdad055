// lz4_paged_read.hip -- the plan and the verdicts of lz4flex_paged_read_ranges, gfx950: m byte ranges of paged streams read in one call,
// with the page table where lz4flex_compress_paged left it -- in device memory -- and no host round trip.  The RULE is stated in
// include/lz4flex_amd.h, its integer part is paged_range.h (the functions the MEM_HOST path and the CPU tests run), and
// tests/paged_read_model.py is the same rule as a program.
//
// The decode itself is lz4flex_decompress_batch_partial in MEM_DEVICE, twice (capi.cpp paged_read_on_device): the bodies straight into
// the output, the heads into scratch; lz4_packed.hip's offset scan gives every range its item slots and its head slot.  What is here:
//   paged_read_locate_kernel    a LANE per range: two binary searches over the stream's slice of page_src -> one RangeRec, and the two
//                               sizes the scans sum (touched pages, head bytes);
//   paged_read_check_kernel     a WAVEFRONT per range, behind the scans: is the range served by max_items / scratch_cap, and does every
//                               touched page agree with the rule (paged_range.h page_ok; lanes stride over the pages, one ballot) --
//                               REC_SERVED / REC_BAD.  A range that is not served is not walked;
//   paged_read_emit_kernel      a THREAD per item slot 0 .. max_items - 1: the owning range by a binary search over the scanned slot
//                               offsets, then that page's item -- a body into batch A, a head into batch B and the gather.  A slot nobody
//                               owns and a range without a head get a one-byte block with target 0, which the partial decoder answers
//                               without reading anything (an EMPTY block would go to its second pass);
//   paged_read_verdict_kernel   a WAVEFRONT per range: the first touched page, in stream order, that did not deliver decides.
// No LDS, no atomics, no scratch memory.  Every store is a plain vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4_device.h"
#include "paged_range.h"

namespace lz4flex_dev {

using lz4flex_paged::Item;
using lz4flex_paged::RangeRec;
using lz4flex_paged::REC_BAD;
using lz4flex_paged::REC_HEAD;
using lz4flex_paged::REC_NO_STREAM;
using lz4flex_paged::REC_SERVED;

size_t paged_read_work_bytes(uint32_t m, uint32_t max_items) {
    const size_t r = m, t = max_items;
    return up256(sizeof(RangeRec) * r) + 2u * up256(8u * r) + 2u * up256(8u * (r + 1u)) + up256(8u * scan_tiles(m)) +
           2u * up256(8u * t) + 4u * up256(4u * t) + 4u * up256(8u * r) + 5u * up256(4u * r);
}

PagedReadWork paged_read_work(void* work, uint32_t m, uint32_t max_items) {
    const size_t r = m, t = max_items;
    uint8_t* p = (uint8_t*)work;
    PagedReadWork w;
    w.rec = (RangeRec*)p; p += up256(sizeof(RangeRec) * r);
    w.nb = (uint64_t*)p; p += up256(8u * r);
    w.hb = (uint64_t*)p; p += up256(8u * r);
    w.slot = (uint64_t*)p; p += up256(8u * (r + 1u));
    w.head_off = (uint64_t*)p; p += up256(8u * (r + 1u));
    w.tiles = (uint64_t*)p; p += up256(8u * scan_tiles(m));
    w.a_in = (uint64_t*)p; p += up256(8u * t);
    w.a_out = (uint64_t*)p; p += up256(8u * t);
    w.a_len = (uint32_t*)p; p += up256(4u * t);
    w.a_tgt = (uint32_t*)p; p += up256(4u * t);
    w.a_olen = (uint32_t*)p; p += up256(4u * t);
    w.a_st = (int32_t*)p; p += up256(4u * t);
    w.b_in = (uint64_t*)p; p += up256(8u * r);
    w.b_out = (uint64_t*)p; p += up256(8u * r);
    w.d_src = (uint64_t*)p; p += up256(8u * r);
    w.d_dst = (uint64_t*)p; p += up256(8u * r);
    w.b_len = (uint32_t*)p; p += up256(4u * r);
    w.b_tgt = (uint32_t*)p; p += up256(4u * r);
    w.b_olen = (uint32_t*)p; p += up256(4u * r);
    w.b_st = (int32_t*)p; p += up256(4u * r);
    w.d_len = (uint32_t*)p;
    return w;
}

__global__ void __launch_bounds__(256) paged_read_locate_kernel(PagedReadArgs a, PagedReadWork w) {
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.m; r += (uint64_t)gridDim.x * blockDim.x) {
        RangeRec q;
        lz4flex_paged::locate(a.t, a.range_stream[r], a.range_off[r], a.range_len[r], &q);
        w.rec[r] = q;
        w.nb[r] = q.nb;
        w.hb[r] = q.head_bytes;
    }
}

// four wavefronts, four ranges per workgroup
__global__ void __launch_bounds__(256) paged_read_check_kernel(PagedReadArgs a, PagedReadWork w) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t r = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= a.m) return;
    const RangeRec q = w.rec[r];
    if (q.len == 0u) return;                                                             // nothing wanted: no flag is read
    if (!lz4flex_paged::served(q, w.slot[r], w.head_off[r], a.max_items, a.scratch_cap)) return;
    bool ok = true;
    if ((q.flags & REC_BAD) == 0u)
        for (uint32_t j = lane; j < q.nb && ok; j += 64u) ok = lz4flex_paged::page_ok(a.t, q, q.j0 + j);
    const bool all_ok = __ballot(!ok) == 0ull;
    if (lane == 0u) w.rec[r].flags = q.flags | REC_SERVED | (all_ok ? 0u : REC_BAD);
}

// the range item slot t belongs to: the LAST r with slot[r] <= t (ranges without pages share their slot with the range behind them)
__device__ __forceinline__ uint32_t range_of_slot(const uint64_t* __restrict__ slot, uint32_t m, uint64_t t) {
    uint32_t lo = 0u, hi = m;                          // slot[lo] <= t; hi == m or slot[hi] > t
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (slot[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool planned(uint32_t flags) { return (flags & (REC_SERVED | REC_BAD | REC_NO_STREAM)) == REC_SERVED; }

// Thread t < max_items writes slot t of batch A; the thread of a planned range's first slot writes the range's entries of batch B and of
// the gather when the range has a head, thread r < m writes them (empty) for every other range r.
__global__ void __launch_bounds__(256) paged_read_emit_kernel(PagedReadArgs a, PagedReadWork w, uint64_t threads) {
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < threads; t += (uint64_t)gridDim.x * blockDim.x) {
        if (t < a.m) {
            const uint32_t f = w.rec[t].flags;
            if (!planned(f) || (f & REC_HEAD) == 0u) {
                w.b_in[t] = 0ull; w.b_len[t] = 1u; w.b_out[t] = 0ull; w.b_tgt[t] = 0u;
                w.d_src[t] = 0ull; w.d_dst[t] = 0ull; w.d_len[t] = 0u;
            }
        }
        if (t >= a.max_items) continue;
        const uint32_t r = range_of_slot(w.slot, a.m, t);
        const RangeRec q = w.rec[r];
        const uint64_t j = t - w.slot[r];
        Item it;
        const bool own = planned(q.flags) && j < q.nb;
        const bool have = own && lz4flex_paged::item_of(a.t, q, q.j0 + (uint32_t)j, a.out_off[r], w.head_off[r], &it);
        const bool body = have && !it.head;
        w.a_in[t] = body ? it.in_off : 0ull; w.a_len[t] = body ? it.in_len : 1u;
        w.a_out[t] = body ? it.out_off : 0ull; w.a_tgt[t] = body ? it.target : 0u;
        if (own && j == 0ull && (q.flags & REC_HEAD) != 0u) {
            const bool head = have && it.head;
            w.b_in[r] = head ? it.in_off : 0ull; w.b_len[r] = head ? it.in_len : 1u;
            w.b_out[r] = head ? it.out_off : 0ull; w.b_tgt[r] = head ? it.target : 0u;
            w.d_src[r] = head ? it.out_off + it.copy_at : 0ull; w.d_dst[r] = head ? a.out_off[r] : 0ull; w.d_len[r] = head ? it.copy_len : 0u;
        }
    }
}

// status[r] / out_len[r] in the header's order: no such stream, nothing wanted, not served, a contradicting table, then the first
// touched page, in stream order, that failed to decode or decoded to fewer bytes than wanted
__global__ void __launch_bounds__(256) paged_read_verdict_kernel(PagedReadArgs a, PagedReadWork w) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t r = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= a.m) return;
    const RangeRec q = w.rec[r];
    int32_t st = 0;
    bool walk = false;
    if ((q.flags & REC_NO_STREAM) != 0u) st = lz4flex_paged::E_INVALID_ARG;
    else if (q.len == 0u) st = 0;
    else if ((q.flags & REC_SERVED) == 0u) st = lz4flex_paged::E_OUTPUT_TOO_SMALL;
    else if ((q.flags & REC_BAD) != 0u) st = lz4flex_paged::E_INVALID_ARG;
    else walk = true;
    if (walk) {
        const uint64_t slot = w.slot[r];
        const bool has_head = (q.flags & REC_HEAD) != 0u;
        uint32_t bad_j = 0xFFFFFFFFu;
        int32_t code = 0;
        for (uint32_t j = lane; j < q.nb; j += 64u) {
            const bool head = has_head && j == 0u;
            const int32_t v = head ? lz4flex_paged::item_verdict(w.b_st[r], w.b_olen[r], w.b_tgt[r])
                                   : lz4flex_paged::item_verdict(w.a_st[slot + j], w.a_olen[slot + j], w.a_tgt[slot + j]);
            // (a slot of a planned range whose item was withheld has target 0 where the rule wants bytes: counted as a contradiction)
            const bool withheld = (head ? w.b_tgt[r] : w.a_tgt[slot + j]) == 0u;
            if (v != 0 || withheld) { bad_j = j; code = v != 0 ? v : lz4flex_paged::E_INVALID_ARG; break; }
        }
        uint32_t first = bad_j;
        for (int d = 32; d > 0; d >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)first, d, 64);
            first = o < first ? o : first;
        }
        if (first != 0xFFFFFFFFu) {
            if (bad_j == first) { a.status[r] = code; a.out_len[r] = 0u; }
            return;
        }
    }
    if (lane == 0u) { a.status[r] = st; a.out_len[r] = st == 0 ? q.len : 0u; }
}

hipError_t launch_paged_read_locate(const PagedReadArgs& a, const PagedReadWork& w, hipStream_t s) {
    if (a.m == 0u) return hipSuccess;
    hipLaunchKernelGGL(paged_read_locate_kernel, dim3(grid_of(((uint64_t)a.m + 255u) / 256u)), dim3(256), 0, s, a, w);
    return hipGetLastError();
}

hipError_t launch_paged_read_plan(const PagedReadArgs& a, const PagedReadWork& w, hipStream_t s) {
    if (a.m == 0u) return hipSuccess;
    const uint64_t threads = a.max_items > a.m ? a.max_items : a.m;
    hipLaunchKernelGGL(paged_read_check_kernel, dim3((a.m + 3u) / 4u), dim3(256), 0, s, a, w);
    hipLaunchKernelGGL(paged_read_emit_kernel, dim3(grid_of((threads + 255u) / 256u)), dim3(256), 0, s, a, w, threads);
    return hipGetLastError();
}

hipError_t launch_paged_read_verdict(const PagedReadArgs& a, const PagedReadWork& w, hipStream_t s) {
    if (a.m == 0u) return hipSuccess;
    hipLaunchKernelGGL(paged_read_verdict_kernel, dim3((a.m + 3u) / 4u), dim3(256), 0, s, a, w);
    return hipGetLastError();
}

}  // namespace lz4flex_dev
