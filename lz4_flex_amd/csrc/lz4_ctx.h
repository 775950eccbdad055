// lz4_ctx.h -- the host layer's private state: struct lz4flex_ctx (opaque in include/lz4flex_amd.h) and the few helpers every host file
// that works on a context needs (capi.cpp, frame_many.cpp; sharded.cpp: Desc alone).  Host only, not installed, no kernel includes it.
// Descriptor columns are declared in ONE way, ColumnPlan (lz4_host_stage.h: typed Col<T>, up before down), and two helpers own the memory
// behind a plan: Desc, below, is a pageable image whose device memory the caller owns (a scratch slot, an allocation of its own) -- the
// frame layer, which holds several at once and names its columns in frame_cols.h; HostStage (lz4_host_stage.h) is the context's ONE
// page-locked buffer and arena, with the arena's data regions -- capi.cpp's MEM_HOST calls, one at a time per context.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "lz4_host_stage.h"

namespace lz4flex_dev {

// Descriptor and result columns of one call at 64-byte starts: a column plan, its host image and its device copy.  The caller owns
// the device memory (frame_many.cpp: context scratch slot 0; sharded.cpp: an allocation of its own) and maps the hipError_t.  The
// image grows, zeroed, to the columns declared so far whenever it is touched: a host pointer is not kept across a later declaration.
struct Desc : ColumnPlan {
    std::vector<uint8_t> h;
    uint8_t* d = nullptr;
    Desc() : ColumnPlan(64) {}
    uint8_t* image() { if (h.size() < total()) h.resize(total(), 0); return h.data(); }
    template <class T> T* host(Col<T> c) { return view(image(), c); }
    template <class T> T* dev(Col<T> c) const { return view(d, c); }
    template <class T, class U> void fill(Col<T> c, const U* src) {
        static_assert(sizeof(T) == sizeof(U), "a column takes its caller's array as it is");
        if (c.count) memcpy(host(c), src, sizeof(T) * c.count);
    }
    // the image's first `n` bytes (up_bytes, or total(): what the device only writes lies behind up_bytes) to `dev_mem`, which holds total()
    hipError_t upload(void* dev_mem, size_t n, hipStream_t s) {
        d = (uint8_t*)dev_mem;
        return n ? hipMemcpyAsync(d, image(), n, hipMemcpyHostToDevice, s) : hipSuccess;
    }
    template <class T> hipError_t fetch(Col<T> c, size_t count, hipStream_t s) {
        return count ? hipMemcpyAsync(image() + c.at, d + c.at, count * sizeof(T), hipMemcpyDeviceToHost, s) : hipSuccess;
    }
    template <class T> hipError_t fetch_columns(Col<T> first, hipStream_t s) {      // from this column to the end, one copy
        return hipMemcpyAsync(image() + first.at, d + first.at, from(first), hipMemcpyDeviceToHost, s);
    }
};

// the calling thread's device for the lifetime of the guard: the context's one (err: what selecting it answered)
struct DeviceGuard {
    int prev = 0;
    hipError_t err;
    explicit DeviceGuard(int dev) { (void)hipGetDevice(&prev); err = hipSetDevice(dev); }
    ~DeviceGuard() { (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// grow-only staging memory, device or page-locked host: a larger request frees and allocates (a quarter on top, at least min_cap)
struct GrowBuf {
    bool pinned;
    size_t min_cap;
    uint8_t* p = nullptr;
    size_t cap = 0;
    void free() { if (p) (void)(pinned ? hipHostFree(p) : hipFree(p)); p = nullptr; cap = 0; }
    hipError_t ensure(size_t need) {
        if (need <= cap) return hipSuccess;
        free();
        const size_t want = std::max<size_t>(need + need / 4, min_cap);
        const hipError_t e = pinned ? hipHostMalloc((void**)&p, want, hipHostMallocDefault) : hipMalloc((void**)&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
};

// A workspace that is ONE per context while MEM_DEVICE batches are enqueued on the caller's stream: two batches on different streams
// could overlap on the GPU and race on it.  acquire() before the first thing enqueued that touches it: a launch on another stream than
// the previous one first makes its stream wait for that one's event (same stream: already ordered).  release() behind the last one.
// The workspace counts as used from acquire() on: a call that fails between the two still leaves work of its stream on it.
struct OrderedWs {
    hipEvent_t done = nullptr;
    hipStream_t last = nullptr;
    bool used = false;
    hipError_t create() { return hipEventCreateWithFlags(&done, hipEventDisableTiming); }
    void destroy() { if (done) (void)hipEventDestroy(done); done = nullptr; }
    hipError_t acquire(hipStream_t s) {
        if (used && s != last) { const hipError_t w = hipStreamWaitEvent(s, done, 0); if (w != hipSuccess) return w; }
        last = s; used = true;
        return hipSuccess;
    }
    hipError_t release(hipStream_t s) { last = s; return hipEventRecord(done, s); }
};

}  // namespace lz4flex_dev

struct lz4flex_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    lz4flex_dev::GrowBuf arena{false, 1u << 20};   // device staging for MEM_HOST calls
    lz4flex_dev::GrowBuf pin{true, 1u << 16};      // pinned host staging for descriptor / result arrays
    lz4flex_dev::GrowBuf pay{true, 1u << 20};      // pinned host staging for compacted results of MEM_HOST compress batches
    int dec_lanes = 16;           // lanes per block, decode
    int comp_lanes = 8;           // lanes per block, encode
    int comp_mode = 0;            // 0 = throughput ("wave") encoder, own parse (default); 1 = reference-exact encoder (lz4_flex's bytes); 2 = high (lz4_compress_high.hip: deep search; which calls keep it and in which form is lz4_route.h encode_route, with the two settings below).  No call writes a setting: lz4flex_set_tuning, the constructor's environment reads and lz4flex_compress_into_with_table's copy are the writers
    int comp_depth = 16;          // "compress_depth": compress_mode 2, the candidates examined per position (1 .. 256)
    int comp_parse = 0;           // "compress_parse": compress_mode 2, 0 = the one-step lazy parse (default), 1 = the optimal parse over the same best[] (tests/sim/high_optimal_model.c's bytes)
    int comp_high_dict = 0;       // "compress_high_dict": compress_mode 2, 1 = calls with dictionaries take the high encoder's dictionary form (tests/sim/high_dict_model.c's bytes); 0 = the throughput encoder (default)
    int comp_high_linked = 0;     // "compress_high_linked": compress_mode 2, 1 = LZ4FLEX_BLOCK_HISTORY bits are read (the block's history is its dictionary: tests/sim/high_dict_model.c's bytes) and Linked frames keep the mode; 0 = the bits are ignored, Linked frames take the throughput encoder (default)
    int comp_high_digest = 1;     // "compress_high_digest": the dictionary form, 1 = a shared dictionary's positions are sorted once per call; 0 = with every block's own (A/B measurements, tests)
    int comp_variant = 1;         // reference-exact encoder: 1 = group encoder + emitter wave (default), 3 = group encoder alone
    uint8_t* pcd_ws = nullptr;    // workgroup decoder, small batches: a parser and a copier workgroup per block hand token lists over through this (lz4_device.h pair_ws)
    lz4flex_dev::OrderedWs pcd;
    int dec_pcd_pair = 1;         // 1: two workgroups per block for batches of few large blocks; 0: never, 2: whenever the batch is small enough (tests, measurements)
    uint32_t* chain_ws = nullptr; // chained decode batches (Linked frames): one "done" word per block, CHAIN_MAX_BLOCKS of them
    lz4flex_dev::OrderedWs chain;
    void* wave_ws = nullptr;      // wave encoder workspace: wave_wgs persistent workgroups; allocated by lz4flex_ctx_create
    lz4flex_dev::OrderedWs wave;
    unsigned long long* wave_prof = nullptr;   // tools: per-role cycle counters of the wave encoder (lz4flex_debug_wave_prof)
    int wave_wgs = 0;
    int dec_blocks_per_wg = 0;    // split decoder: blocks per workgroup (8/16/32/64), 0 = 64
    int comp_det = 0;             // "compress_deterministic": 1 = a block's bytes depend on the block and the settings alone (no sub-windows by batch size)
    int dec_level_chains = 1024;  // "decompress_level_chains": from this many Linked streams in one *_many call on, block k of every stream is one plain launch (frame_many.cpp); 0 = never
    int comp_sub = 0;             // throughput encoder, "compress_subwindows": 0 = by batch size, 1 = never, 2 / 4 = always that many sub-windows per block of <= 64 KiB
    int dec_variant = 0;          // "decompress_variant": 0 = by batch shape, else a pinned decoder -- the numbers are lz4_route.h's Decoder, what each one runs is DECODER_VARIANTS, which batch takes which is decode_route
    int comp_sliding = 2;         // throughput encoder: the windows of a block longer than 64 KiB advance by 48 KiB (2: every window start has 16 KiB of history) or 32 KiB (1: round 4's bytes); 0 = by 64 KiB (round 3's bytes, fastest)
    int comp_carry_wait = 1;      // tests: 0 = a window of the throughput encoder that has to wait for its predecessor's carry gives up at once (the block then takes the second launch)
    int dec_second_pass = 1;      // tests: 0 leaves the blocks a first-pass decoder marked (status DECODE_REDO) instead of decoding them again
    // plan / replay decoder (lz4_decompress_plan.hip, lz4_decompress_replay.hip): the copy plans of a batch, plan_slot_words() words per
    // block + a 32-byte header each.  Grows with the largest batch seen (a hipMalloc -- a device synchronisation -- in the first such
    // call and whenever a larger batch arrives; never shrinks).
    uint8_t* plan_ws = nullptr;
    size_t plan_cap = 0;
    lz4flex_dev::OrderedWs plan;
    int chain_giveup = 0;         // tests: block chain_giveup - 1 of the next chained decode batches gives up without an error (the ordered second pass decodes it and everything behind it)
    int exact_dict_piece = 0;     // tests: the reference-exact encoder's dictionary calls build their chain records in pieces of at most this many blocks (0: as many as the workspace holds)
    // many frames at once (frame_many.cpp): device scratch of the calls that run to completion before they return (compressed staging,
    // descriptor arrays, staged host buffers).  Grow-only, a hipMalloc when a larger job arrives; freed with the context.
    void* many_ws[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t many_cap[4] = {0, 0, 0, 0};
    int fail_next_batch = 0;      // tests: the next N batch calls on this context fail before they launch anything (what an allocation failure looks like to the caller)
    int comp_shared = 1;          // "compress_shared_dict": 1 = lz4flex_compress_batch_shared_dict starts its items from the dictionary's digest; 0 = every item takes the per-block path (A/B measurements, tests)
    bool shared_counted = false;  // the last shared-dictionary call ran the throughput encoder: its digest counter is what "debug_shared_dict_items" reads
    const struct lz4flex_dict_set* set_counted = nullptr;   // the set of the last lz4flex_compress_batch_dict_set call that ran the throughput encoder: what "debug_dict_set_items" reads (capi.cpp checks that it still exists)
    int dec_shared = 1;           // "decompress_shared_dict": 1 = lz4flex_decompress_batch_shared_dict runs the sequence decoder's dictionary form; 0 = every block through decode_block<16, true>, the per-block path (A/B measurements, tests)
    int dec_partial = 1;          // "decompress_partial": 1 = lz4flex_decompress_batch_partial runs the sequence decoder's partial form; 0 = every block through decode_block<16, false, true>, the reference's order (A/B measurements, tests)
    int packed_tile = 0;          // "packed_scan_tile" (read-only): the sizes one workgroup of the packed entries' offset scan takes
    int range_pass_bytes = 256 << 20;   // "frame_range_pass_bytes": lz4flex_frame_read_ranges cuts its ranges into passes whose scratch (heads; MEM_HOST: the staged spans and outputs too) stays under this; a pass takes at least one range
    int range_checksums = 1;      // "frame_range_checksums": 1 = a range read verifies the block checksums of the blocks it touches (frames that have them); 0 = not (A/B measurements, tests)
    int size_serial = 0;          // "size_scan_serial": 1 = lz4flex_decompressed_size_batch measures every block with its serial (reference-order) pass (tests)
    int fit_serial = 0;           // "fit_serial": 1 = lz4flex_fit_batch / lz4flex_compress_batch_fit cut every block with the serial (reference-order) pass (tests, A/B)
    int fit_first_pass = 0;       // "debug_fit_first_pass" (test hook): 1 = the fit entries run their wavefront pass alone, the blocks it gives up stay marked FIT_REDO
    int filter_bytewise = 0;      // "filter_bytewise": 1 = the shuffle / bitshuffle kernels (lz4_filter.hip) take every block by their narrow path, byte accesses (A/B measurements, tests)
};

namespace lz4flex_dev {
// capi.cpp, for frame_many.cpp: *ctx = the calling thread's default context if null; grow-only device scratch in 4 slots (valid until
// the next ctx_scratch of the same slot; the caller runs to completion before it returns)
int ctx_resolve(lz4flex_ctx** ctx);
int ctx_scratch(lz4flex_ctx* c, int slot, size_t bytes, void** out);
}  // namespace lz4flex_dev
