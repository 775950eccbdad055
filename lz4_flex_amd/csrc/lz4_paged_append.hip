// lz4_paged_append.hip -- the plan and the resume step of lz4flex_paged_append, gfx950: new bytes for any subset of n paged streams in one
// call, the tail page of every such stream reopened, with the tables where lz4flex_compress_paged left them -- in device memory -- and no
// host round trip.  The RULE is stated in include/lz4flex_amd.h, its integer part is paged_append.h (the functions the MEM_HOST path and
// the CPU tests run), and tests/paged_append_model.py is the same rule as a program.
//
// The reopen is lz4flex_decompress_batch_partial in MEM_DEVICE over n tail items and launch_copy_batch over n add items (capi.cpp
// paged_append_on_device); lz4_packed.hip's offset scan gives every stream its stage slot; the rounds behind the resume step are those of
// lz4flex_compress_paged, unchanged (lz4_paged.hip paged_step_kernel with PAGED_NEXT / PAGED_LAST).  What is here, a LANE per stream each:
//   paged_append_locate_kernel  steps 1 to 3 of the rule (paged_append.h append_locate) -> one AppendRec, and the slot size the scan sums;
//   paged_append_emit_kernel    behind the scan: is the stream served by stage_cap -- APP_SERVED, stage_off, tail_src --, then its tail item
//                               (page -> slot, target T) and its copy item (add -> slot + T).  A stream that is dead, and a fresh stream
//                               without a tail, get a one-byte block with target 0, which the partial decoder answers without reading
//                               anything, and a copy of length 0;
//   paged_append_resume_kernel  behind the decode and the copy, in the place of the PAGED_FIRST step: the verdict of the tail decode, then
//                               pos = base, k = k - 1, W = window_min for the streams that go on, round 1 laid out in the PagedWork arrays,
//                               and the in_off' / in_len' the following steps read: the stage position of stream byte 0 (stage_off - base,
//                               modulo 2^64) and S + A.  With max_rounds == 0 it ends what is live, as PAGED_FIRST | PAGED_LAST does.
// Offsets are 64-bit throughout.  No LDS, no atomics, no scratch memory; VGPRs: locate 24, emit 26, resume 36.  Every store is a
// plain vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4_device.h"
#include "paged_append.h"

namespace lz4flex_dev {

using lz4flex_paged::APP_BAD;
using lz4flex_paged::APP_IDLE;
using lz4flex_paged::APP_SERVED;
using lz4flex_paged::AppendRec;
using lz4flex_paged::AppendTables;

size_t paged_append_work_bytes(uint32_t n) {
    const size_t m = n;
    return up256(paged_work_bytes(n)) + up256(sizeof(AppendRec) * m) + up256(8u * m) + up256(8u * (m + 1u)) + up256(8u * scan_tiles(n)) +
           5u * up256(8u * m) + 6u * up256(4u * m);
}

PagedAppendWork paged_append_work(void* work, uint32_t n) {
    const size_t m = n;
    uint8_t* p = (uint8_t*)work;
    PagedAppendWork w;
    w.paged = p; p += up256(paged_work_bytes(n));
    w.rec = (AppendRec*)p; p += up256(sizeof(AppendRec) * m);
    w.need = (uint64_t*)p; p += up256(8u * m);
    w.slot = (uint64_t*)p; p += up256(8u * (m + 1u));
    w.tiles = (uint64_t*)p; p += up256(8u * scan_tiles(n));
    w.t_in = (uint64_t*)p; p += up256(8u * m);
    w.t_out = (uint64_t*)p; p += up256(8u * m);
    w.c_src = (uint64_t*)p; p += up256(8u * m);
    w.c_dst = (uint64_t*)p; p += up256(8u * m);
    w.v_off = (uint64_t*)p; p += up256(8u * m);
    w.t_len = (uint32_t*)p; p += up256(4u * m);
    w.t_tgt = (uint32_t*)p; p += up256(4u * m);
    w.t_olen = (uint32_t*)p; p += up256(4u * m);
    w.t_st = (int32_t*)p; p += up256(4u * m);
    w.c_len = (uint32_t*)p; p += up256(4u * m);
    w.v_len = (uint32_t*)p;
    return w;
}

__device__ __forceinline__ AppendTables tables_of(const PagedAppendArgs& a) {
    return AppendTables{a.page_off, a.page_len, a.page_src, a.n_pages, a.in_done, a.n, a.page_size, a.window_max};
}

__global__ void __launch_bounds__(256) paged_append_locate_kernel(PagedAppendArgs a, PagedAppendWork w) {
    const AppendTables t = tables_of(a);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * blockDim.x) {
        AppendRec q;
        lz4flex_paged::append_locate(t, (uint32_t)i, a.add_len[i], &q);
        w.rec[i] = q;
        w.need[i] = lz4flex_paged::append_slot_bytes(q);
    }
}

__global__ void __launch_bounds__(256) paged_append_emit_kernel(PagedAppendArgs a, PagedAppendWork w) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * blockDim.x) {
        const AppendRec q = w.rec[i];
        const uint64_t slot = w.slot[i];
        const bool go = lz4flex_paged::append_pre(q, slot, a.stage_cap) == -1;
        if (go) w.rec[i].flags = q.flags | APP_SERVED;
        a.stage_off[i] = go ? slot : lz4flex_paged::NO_STAGE;
        a.tail_src[i] = (q.flags & (APP_IDLE | APP_BAD)) != 0u ? q.S : q.base;
        const bool tail = go && q.T != 0u;
        const uint64_t e = q.first + lz4flex_paged::append_k0(q);
        w.t_in[i] = tail ? e * (uint64_t)a.page_size : 0ull;
        w.t_len[i] = tail ? a.page_len[e] : 1u;
        w.t_out[i] = tail ? slot : 0ull;
        w.t_tgt[i] = tail ? q.T : 0u;
        w.c_src[i] = go ? a.add_off[i] : 0ull;
        w.c_dst[i] = go ? slot + q.T : 0ull;
        w.c_len[i] = go ? q.A : 0u;
    }
}

__global__ void __launch_bounds__(256) paged_append_resume_kernel(PagedAppendArgs a, PagedAppendWork w, PagedWork pw, int32_t no_rounds) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * blockDim.x) {
        const AppendRec q = w.rec[i];
        int32_t st;
        if ((q.flags & APP_IDLE) != 0u) st = 0;
        else if ((q.flags & APP_BAD) != 0u) st = lz4flex_paged::E_INVALID_ARG;
        else if ((q.flags & APP_SERVED) == 0u) st = lz4flex_paged::E_OUTPUT_TOO_SMALL;
        else st = q.T != 0u ? lz4flex_paged::item_verdict(w.t_st[i], w.t_olen[i], q.T) : 0;
        const bool resumed = st == 0 && (q.flags & APP_IDLE) == 0u;      // the stream's tables are the rounds' from here on
        bool live = resumed;
        const uint32_t k0 = lz4flex_paged::append_k0(q);
        if (live && (lz4flex_paged::append_room(q) == 0ull || no_rounds != 0)) { live = false; st = lz4flex_paged::E_OUTPUT_TOO_SMALL; }
        if (resumed) { a.n_pages[i] = k0; a.in_done[i] = q.base; }
        a.status[i] = st;
        const uint64_t slot = w.slot[i];
        const uint32_t W = a.window_min, len = q.T + q.A;
        w.v_off[i] = resumed ? slot - (uint64_t)q.base : 0ull;
        w.v_len[i] = resumed ? q.S + q.A : 0u;
        pw.win[i] = W; pw.live[i] = live ? 1u : 0u;
        pw.w_off[i] = live ? slot : 0ull;
        pw.w_len[i] = live ? (W < len ? W : len) : 0u;
        pw.o_off[i] = live ? (q.first + k0) * (uint64_t)a.page_size : 0ull;
        pw.o_cap[i] = live ? a.page_size : 0u;
    }
}

hipError_t launch_paged_append_locate(const PagedAppendArgs& a, const PagedAppendWork& w, hipStream_t s) {
    if (a.n == 0u) return hipSuccess;
    hipLaunchKernelGGL(paged_append_locate_kernel, dim3(grid_of(((uint64_t)a.n + 255u) / 256u)), dim3(256), 0, s, a, w);
    return hipGetLastError();
}

hipError_t launch_paged_append_emit(const PagedAppendArgs& a, const PagedAppendWork& w, hipStream_t s) {
    if (a.n == 0u) return hipSuccess;
    hipLaunchKernelGGL(paged_append_emit_kernel, dim3(grid_of(((uint64_t)a.n + 255u) / 256u)), dim3(256), 0, s, a, w);
    return hipGetLastError();
}

hipError_t launch_paged_append_resume(const PagedAppendArgs& a, const PagedAppendWork& w, bool no_rounds, hipStream_t s) {
    if (a.n == 0u) return hipSuccess;
    hipLaunchKernelGGL(paged_append_resume_kernel, dim3(grid_of(((uint64_t)a.n + 255u) / 256u)), dim3(256), 0, s, a, w, paged_work(w.paged, a.n), (int32_t)(no_rounds ? 1 : 0));
    return hipGetLastError();
}

}  // namespace lz4flex_dev
