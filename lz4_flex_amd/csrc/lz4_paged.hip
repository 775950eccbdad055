// lz4_paged.hip -- the step between two rounds of lz4flex_compress_paged, gfx950: n streams cut into pages of page_size bytes, every page
// a self-contained LZ4 block that holds as much of its stream as fits (the LZ4_compress_destSize loop of fixed-output compression),
// with no host round trip between pages.  The RULE is stated in include/lz4flex_amd.h and, as a program, in tests/paged_model.py.
//
// A round is the unchanged fit entry (capi.cpp compress_fit_on_device: size pass, offset scan, encoder, fit pass) over one window per
// stream; paged_step_kernel runs in front of the first round, between two rounds and behind the last one, a LANE per stream:
//   * COMMIT the round behind it from that round's out_len / in_used / status (w.r_*): a failed window ends its stream with that status;
//     a window that fit whole, with more of the stream behind it and a window that can still grow, is offered again at twice the
//     length and nothing is committed; else the page is entered into the table (page_len, page_src), pos and k advance, and the stream
//     ends when it is used up (status 0) or out of pages (OUTPUT_TOO_SMALL);
//   * LAY OUT the next round in the workspace: window offset in_off[i] + pos, window length min(W, in_len[i] - pos), output offset
//     (page_off[i] + k) * page_size, capacity page_size.  A stream that is not live gets window length 0 and capacity 0: the fit pass
//     writes nothing at capacity 0 and the next step does not look at its result.
// The stream's state lives in the caller's result arrays (pos = in_done[i], k = n_pages[i]) and in the workspace (W, live); status[i] is 0
// while a stream is live and final once it is not; the step behind the last round ends what is still live with OUTPUT_TOO_SMALL.
// Offsets are 64-bit throughout (an entry index times the page size, a window's place in in_base).  Writes: table entries of committed
// pages, the three per-stream results, the workspace; nothing else (entries at or behind n_pages[i] stay as they are).  No LDS, no
// atomics, no scratch memory; paged_step_kernel: 32 VGPRs.  Every store is a plain vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4_device.h"

namespace lz4flex_dev {

size_t paged_work_bytes(uint32_t n) {
    const size_t m = n;
    return packed_work_bytes(n) + 2u * up256(8u * m) + 7u * up256(4u * m);
}

PagedWork paged_work(void* work, uint32_t n) {
    const size_t m = n;
    uint8_t* p = (uint8_t*)work;
    PagedWork w;
    w.packed = p; p += packed_work_bytes(n);
    w.w_off = (uint64_t*)p; p += up256(8u * m);
    w.o_off = (uint64_t*)p; p += up256(8u * m);
    w.w_len = (uint32_t*)p; p += up256(4u * m);
    w.o_cap = (uint32_t*)p; p += up256(4u * m);
    w.r_len = (uint32_t*)p; p += up256(4u * m);
    w.r_used = (uint32_t*)p; p += up256(4u * m);
    w.r_st = (int32_t*)p; p += up256(4u * m);
    w.win = (uint32_t*)p; p += up256(4u * m);
    w.live = (uint32_t*)p;
    return w;
}

__global__ void __launch_bounds__(256) paged_step_kernel(PagedArgs a, PagedWork w, int32_t phase) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t len = a.in_len[i];
        const uint64_t first = a.page_off[i], room = a.page_off[i + 1u] - first;      // this stream's entries: [first, first + room)
        uint32_t pos, W, k, live;
        int32_t st = 0;
        if ((phase & PAGED_FIRST) != 0) {
            pos = 0u; W = a.window_min; k = 0u;
            live = len != 0u ? 1u : 0u;
            if (live != 0u && room == 0ull) { live = 0u; st = LZ4FLEX_DEV_E_OUTPUT_TOO_SMALL; }     // (no page to commit into: no round is spent on it)
        } else {
            pos = a.in_done[i]; k = a.n_pages[i]; W = w.win[i]; live = w.live[i];
            if (live == 0u) st = a.status[i];
            else {
                const int32_t rs = w.r_st[i];
                const uint32_t offered = w.w_len[i], used = w.r_used[i];
                if (rs != 0) { st = rs; live = 0u; }
                else if (used == offered && offered < len - pos && W < a.window_max) {       // retry: a larger window may fill the page better
                    const uint64_t twice = 2ull * W;
                    W = twice < a.window_max ? (uint32_t)twice : a.window_max;
                } else {
                    const uint64_t e = first + k;
                    a.page_len[e] = w.r_len[i];
                    a.page_src[e] = pos;
                    pos += used; k += 1u;
                    if (pos == len) live = 0u;
                    else if ((uint64_t)k == room) { live = 0u; st = LZ4FLEX_DEV_E_OUTPUT_TOO_SMALL; }
                }
            }
        }
        const bool last = (phase & PAGED_LAST) != 0;
        if (last && live != 0u) { live = 0u; st = LZ4FLEX_DEV_E_OUTPUT_TOO_SMALL; }     // max_rounds are spent
        a.n_pages[i] = k; a.in_done[i] = pos; a.status[i] = st;
        if (last) continue;
        w.win[i] = W; w.live[i] = live;
        const uint32_t left = len - pos;
        w.w_off[i] = a.in_off[i] + (live != 0u ? pos : 0u);
        w.w_len[i] = live != 0u ? (W < left ? W : left) : 0u;
        w.o_off[i] = live != 0u ? (first + k) * (uint64_t)a.page_size : 0ull;
        w.o_cap[i] = live != 0u ? a.page_size : 0u;
    }
}

hipError_t launch_paged_step(const PagedArgs& a, const PagedWork& w, int phase, hipStream_t s) {
    if (a.n == 0u) return hipSuccess;
    const uint64_t groups = ((uint64_t)a.n + 255u) / 256u;
    hipLaunchKernelGGL(paged_step_kernel, dim3((uint32_t)(groups < (1u << 22) ? groups : (1u << 22))), dim3(256), 0, s, a, w, (int32_t)phase);
    return hipGetLastError();
}

}  // namespace lz4flex_dev
