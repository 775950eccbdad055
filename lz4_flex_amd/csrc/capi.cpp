// capi.cpp -- host side of the C ABI declared in include/lz4flex_amd.h.  There is no CPU codec in this library: every call that
// produces bytes launches a kernel.  How a batched call travels through this file:
//   entry point      checks its arguments in ITS order (batch_arrays_ok, classify_mem, begin_batch / injected_failure), describes the
//                    batch as a BatchCall (batch_of: the arrays every batch has; the rest by field name) and hands it to run_batch;
//   run_host_batch   MEM_HOST: mirrors the caller's layout in the context's device arena, rebases the BatchCall onto it, launches,
//                    copies the results back (run_host_small: the one-transfer-each-way form for a few small blocks, which the
//                    lz4_flex-shaped scalar calls -- 1-block batches -- take);
//   run_device_batch MEM_DEVICE: the caller's BatchCall as it is, on the caller's stream;
//   launch_batch     ONE place that turns a BatchCall of device pointers into CompressArgs / DecompressArgs: launch_encode
//                    (launch_compress_any: encode_route's choice, then that mode's launches) and launch_decode (the chain bracket,
//                    decode_route's choice, then launch_first_pass -- that decoder's workspaces and kernels -- and launch_redo, the
//                    second pass behind every first-pass decoder); dict_source_of describes the batch's dictionaries (DictSource)
//                    for both.  Which kernel a batch takes is decided in lz4_route.h alone: pure functions, tested on the CPU.
// The context and the helpers shared with frame_many.cpp (OrderedWs: the rule that orders a per-context workspace across streams;
// DeviceGuard, GrowBuf) are in lz4_ctx.h; how EVERY MEM_HOST call stages its columns and regions is lz4_host_stage.h (HostStage, opened
// on a context by stage_open); the integer settings are one table (SETTINGS) that lz4flex_set_tuning and lz4flex_get_tuning walk.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/lz4flex_amd.h"
#include "lz4_batch_entry.h"
#include "lz4_ctx.h"
#include "lz4_device.h"
#include "lz4_plan_common.h"

using namespace lz4flex_dev;

static thread_local std::string g_last_error;
static thread_local int g_last_hip = 0;

static int hip_fail(hipError_t e, const char* what) {
    g_last_hip = (int)e;
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return -LZ4FLEX_E_HIP;
}
#define HIP_TRY(expr)                                   \
    do {                                                \
        hipError_t _e = (expr);                         \
        if (_e != hipSuccess) return hip_fail(_e, #expr); \
    } while (0)

// NULL context: the calling thread's default one (the scalar calls, the frame layer)
static thread_local lz4flex_ctx* g_default_ctx = nullptr;
static int default_ctx(lz4flex_ctx** out) {
    if (!g_default_ctx) {
        int rc = lz4flex_ctx_create(&g_default_ctx, -1);
        if (rc) return rc;
    }
    *out = g_default_ctx;
    return 0;
}

// A dictionary set (lz4flex_dict_set_create): ONE device allocation -- [table | counter | digests | the kept bytes] -- that nothing writes
// after create but the encoder's counter word.  LIVE_SETS: the sets that exist; "debug_dict_set_items" names the set a context used last
// and must not read one that is gone (a set is not the context's: either may be freed first).
struct lz4flex_dict_set {
    int device = 0;
    uint32_t k = 0;
    uint8_t* mem = nullptr;
    const DictSetRec* table = nullptr;       // device: k records
    uint32_t* counter = nullptr;             // device: the items of the last throughput-encoder call that started from a digest
};
static std::mutex g_sets_mu;
static std::vector<const lz4flex_dict_set*> g_live_sets;
static constexpr uint32_t DICT_SET_MAX = 1024u;
static constexpr uint32_t DICT_KEEP = 65536u;

// tools builds (-DLZ4FLEX_TOOLS) hold the plan / replay and the fused decoder.  plan_fits: BlockPlan's word indices are 32-bit,
// a batch whose plans they cannot address is not the plan / replay decoder's
#ifdef LZ4FLEX_TOOLS
static constexpr bool TOOLS_BUILD = true;
static bool plan_fits(uint32_t n) { return (uint64_t)n * plan_slot_words() <= 0xFFFFFFFFull; }
#else
static constexpr bool TOOLS_BUILD = false;
static bool plan_fits(uint32_t) { return false; }
#endif

// The "done" words of a chained batch are the context's: two chained batches on different streams would clear and poll the same
// flags (ADVICE r3 for the device path, r4 for the host path: ONE helper for both).  The event is recorded behind the memset too: a
// call that fails between here and chain_ws_end still leaves ordered work of this stream on the words.
static hipError_t chain_ws_begin(lz4flex_ctx* c, uint32_t n, hipStream_t s) {
    const hipError_t w = c->chain.acquire(s);
    if (w != hipSuccess) return w;
    const hipError_t m = hipMemsetAsync(c->chain_ws, 0, 4ull * n, s);
    if (m != hipSuccess) return m;
    return c->chain.release(s);
}
static hipError_t chain_ws_end(lz4flex_ctx* c, hipStream_t s) { return c->chain.release(s); }

// The launches of a decode route (lz4_route.h decode_route chose it; nothing here decides).  A batch's form is (d, partial).
// The second pass behind a first-pass decoder: the blocks it left marked DECODE_REDO (errors, sinks too small, shapes it does not
// take) are decoded again in the reference's order of checks, side by side, by the reference-order entry of the batch's form --
// Redo::ChainOrder: a chained batch's marked blocks depend on each other, in chain order.  "decompress_second_pass" 0
// (tests) leaves them marked.
static hipError_t launch_redo(lz4flex_ctx* c, const DecompressArgs& a, Redo redo, const DictSource& d, bool partial, hipStream_t s) {
    if (redo == Redo::None || !c->dec_second_pass) return hipSuccess;
    DecompressArgs r = a;
    r.only_status = DECODE_REDO;
    if (redo == Redo::ChainOrder) return launch_decompress_chain_redo(r, s);
    return launch_decompress(r, d, partial, c->dec_lanes, s);
}

// one block per workgroup (lz4_decompress_pcd.hip).  pair: a parser and a copier workgroup per block; the hand-over workspace is the
// context's: launches on different streams are ordered by an event, as the encoder's are
static hipError_t launch_workgroup(lz4flex_ctx* c, DecompressArgs a, const DecodeRoute& r, hipStream_t s) {
    if (r.pair) {
        const hipError_t w = c->pcd.acquire(s);
        if (w != hipSuccess) return w;
        const hipError_t m = hipMemsetAsync(c->pcd_ws, 0, 64ull * a.n, s);
        if (m != hipSuccess) return m;
        a.pair_ws = c->pcd_ws;
    }
    const hipError_t e = launch_decompress_pcd(a, DECODE_REDO, s, r.pcd_geometry);
    return e == hipSuccess && r.pair ? c->pcd.release(s) : e;
}

#ifdef LZ4FLEX_TOOLS
// plan / replay: every block is turned into a copy plan (one wavefront per block, everything that is parallel), then the plans are
// replayed (four lanes per block, the serial rest); blocks without a plan (errors, sinks too small, oversized) are left to the second pass
static hipError_t launch_plan_replay(lz4flex_ctx* c, const DecompressArgs& a, hipStream_t s) {
    const size_t slot = plan_slot_words();
    const size_t need = (size_t)a.n * (slot * 4u + 32u) + 256u;
    if (need > c->plan_cap) {
        if (c->plan.used) { const hipError_t w = hipEventSynchronize(c->plan.done); if (w != hipSuccess) return w; }
        if (c->plan_ws) (void)hipFree(c->plan_ws);
        c->plan_ws = nullptr; c->plan_cap = 0;
        const hipError_t m = hipMalloc((void**)&c->plan_ws, need);
        if (m != hipSuccess) return m;
        c->plan_cap = need;
    }
    hipError_t e = c->plan.acquire(s);
    if (e != hipSuccess) return e;
    PlanArgs pa;
    pa.in_base = a.in_base; pa.in_off = a.in_off; pa.in_len = a.in_len; pa.out_off = a.out_off; pa.out_cap = a.out_cap;
    pa.plans = (plan::BlockPlan*)c->plan_ws;
    pa.words = (uint32_t*)(c->plan_ws + align_up((size_t)a.n * 32u, 256));
    pa.out_len = a.out_len; pa.status = a.status; pa.n = a.n; pa.slot_words = (uint32_t)slot; pa.redo_code = DECODE_REDO;
    e = launch_plan(pa, s);
    if (e != hipSuccess) return e;
    ReplayArgs ra;
    ra.in_base = a.in_base; ra.out_base = a.out_base; ra.plans = pa.plans; ra.words = pa.words; ra.n = a.n; ra.max_turns = (uint32_t)(slot / plan::TURN_WORDS) + 2u;
    e = launch_replay(ra, s);
    if (e != hipSuccess) return e;
    e = c->plan.release(s);
    if (e != hipSuccess) return e;
    return a.detail ? hipMemsetAsync(a.detail, 0, 16ull * a.n, s) : hipSuccess;
}
#endif

// the route's decoder over the batch: a first pass that marks what it leaves, or -- DEC_REFERENCE -- every block in the reference's order
static hipError_t launch_first_pass(lz4flex_ctx* c, const DecompressArgs& a, const DecodeRoute& r, const DictSource& d, bool partial, hipStream_t s) {
    switch (r.decoder) {
        case DEC_REFERENCE: return launch_decompress(a, d, partial, c->dec_lanes, s);
        case DEC_WORKGROUP: return launch_workgroup(c, a, r, s);
        case DEC_SEQUENCE: return launch_decompress_seq(a, d, partial, DECODE_REDO, s);
        case DEC_SPLIT: return launch_decompress_split(a, s, c->dec_blocks_per_wg);
#ifdef LZ4FLEX_TOOLS
        case DEC_PLAN: return launch_plan_replay(c, a, s);
        case DEC_FUSED: return launch_decompress_fused(a, DECODE_REDO, s);
#endif
        default: return hipErrorInvalidValue;      // (decode_route names no decoder this build lacks)
    }
}

// MEM_HOST batches whose results are sparse in the output span (compress: ~15 KB used of every 72 KB stride):
// pack the produced bytes densely on the device so that ONE transfer brings them to the host.
__global__ void __launch_bounds__(256) lz4flex_pack_results_kernel(const uint8_t* src, const uint64_t* src_off, const uint32_t* len,
                                                                   const int32_t* status, const uint64_t* dst_off, uint8_t* dst,
                                                                   uint32_t n) {
    const uint32_t b = blockIdx.x;
    if (b >= n || status[b] != 0) return;
    const uint8_t* s = src + src_off[b];
    uint8_t* d = dst + dst_off[b];
    const uint32_t m = len[b];
    for (uint32_t i = threadIdx.x; i < m; i += 256u) d[i] = s[i];
}

// staging memory that has to hold `need` bytes; a failed allocation is this thread's last error like every other HIP failure
static int ensure_buf(GrowBuf& b, size_t need) {
    const hipError_t e = b.ensure(need);
    return e == hipSuccess ? 0 : hip_fail(e, b.pinned ? "hipHostMalloc (staging)" : "hipMalloc (staging)");
}

// a MEM_HOST call's plan (lz4_host_stage.h) onto the context: the page-locked buffer holds the column image, the arena the regions
static int stage_open(lz4flex_ctx* c, HostStage& st) {
    int rc;
    if ((rc = ensure_buf(c->pin, st.total()))) return rc;
    if ((rc = ensure_buf(c->arena, st.arena_bytes))) return rc;
    st.hp = c->pin.p; st.d = c->arena.p; st.s = c->stream;
    return 0;
}

// the throughput encoder's workspace (it also holds the reference-exact mode's dictionary chain records): ordered across streams
static int wave_ws_acquire(lz4flex_ctx* c, hipStream_t s) {
    if (!c->wave_ws || !c->wave.done) { g_last_error = "context without encoder workspace"; return -LZ4FLEX_E_INVALID_ARG; }
    HIP_TRY(c->wave.acquire(s));
    return 0;
}

static int launched(hipError_t le) { return le != hipSuccess ? hip_fail(le, "kernel launch") : 0; }

// mode 2: its scratch is the (otherwise idle) throughput encoder's workspace, ordered across streams like that encoder's own launches;
// a workgroup holds most of a CU's LDS, so one per CU (wave_wgs is two per CU) and no more than the workspace has slices for
static int compress_high(lz4flex_ctx* c, const CompressArgs& a, const DictSource& d, HighForm form, hipStream_t s) {
    if (const int rc = wave_ws_acquire(c, s)) return rc;
    const size_t bytes = compress_wave_workspace_bytes(c->wave_wgs);
    const int wgs = c->wave_wgs / 2;
    const uint32_t depth = (uint32_t)c->comp_depth, parse = (uint32_t)c->comp_parse;
    hipError_t le = form == HighForm::History ? launch_compress_high_linked(a, c->wave_ws, bytes, wgs, depth, parse, s)
                    : form == HighForm::Dict  ? launch_compress_high_dict(a, d, c->comp_high_digest != 0, c->wave_ws, bytes, wgs, depth, parse, s)
                                              : launch_compress_high(a, c->wave_ws, bytes, wgs, depth, parse, s);
    const hipError_t re = c->wave.release(s);
    return launched(le == hipSuccess ? re : le);
}

// mode 0: the throughput encoder (own parse, any block length)
static int compress_throughput(lz4flex_ctx* c, const CompressArgs& a, const DictSource& d, hipStream_t s) {
    if (const int rc = wave_ws_acquire(c, s)) return rc;
    if (d.has_set) HIP_TRY(hipMemsetAsync(d.set.counter, 0, 4, s));      // ("debug_dict_set_items" speaks of this call)
    CompressArgs aw = a;
    aw.slide = c->comp_sliding == 2 ? 49152u : (c->comp_sliding == 1 ? 32768u : 0u);
    // sub-windows (lz4_compress_wave.hip Item::sub): batches that leave at least half / three quarters of the persistent workgroups
    // without a block cut their blocks of <= 64 KiB into 2 / 3 / 4 items each
    aw.sub = c->comp_det ? 1u : c->comp_sub != 0 ? (uint32_t)c->comp_sub
                              : (a.n * 4u <= (uint32_t)c->wave_wgs ? 4u : (a.n * 3u <= (uint32_t)c->wave_wgs ? 3u : (a.n * 2u <= (uint32_t)c->wave_wgs ? 2u : 1u)));
    SharedDictArgs sh{};
    sh.dict = d.shared; sh.len = d.shared_len; sh.use = (uint32_t)c->comp_shared;
    const hipError_t le = launch_compress_wave(aw, c->wave_ws, c->wave_wgs, s, c->wave_prof, c->comp_carry_wait != 0, d.shared ? &sh : nullptr,
                                               d.has_set ? &d.set : nullptr);
    if (le == hipSuccess) HIP_TRY(c->wave.release(s));
    return launched(le);
}

// mode 1: the reference-exact encoder (lz4_compress.hip launch_compress_exact).  A call with dictionaries builds its chain records in
// the (otherwise idle) throughput encoder's workspace: no allocation, ordered across streams like that encoder's own launches
static int compress_exact(lz4flex_ctx* c, const CompressArgs& a, const DictSource& d, bool big, hipStream_t s) {
    const bool emitter = c->comp_variant == 1;     // "compress_variant": 1 = encode_block + emitter wavefront (default), 3 = encode_block alone
    if (!((a.dict_len || d.shared || d.has_set) && a.n)) return launched(launch_compress_exact(a, d, c->comp_lanes, big, emitter, nullptr, 0, 0, s));
    if (const int rc = wave_ws_acquire(c, s)) return rc;
    const hipError_t le = launch_compress_exact(a, d, c->comp_lanes, big, emitter, c->wave_ws, compress_wave_workspace_bytes(c->wave_wgs),
                                                (uint32_t)c->exact_dict_piece, s);
    const hipError_t re = c->wave.release(s);                 // (also behind a failed launch: whatever was enqueued on the workspace is ordered)
    return launched(le == hipSuccess ? re : le);
}

// the encoders for independent blocks.  d: the batch's shared dictionary or set (a has no dictionaries and no flags then), or neither;
// set: the handle behind d.set (null without one); linked_frame: the frame layer's statement about the call.  Which encoder: lz4_route.h
static int launch_compress_any(lz4flex_ctx* c, const CompressArgs& a, const DictSource& d, const lz4flex_dict_set* set, bool big, bool linked_frame,
                               hipStream_t s) {
    const EncodeRoute enc = encode_route(EncodeSettings{c->comp_mode, c->comp_high_dict, c->comp_high_linked},
                                         EncodeShape{a.dict_len || d.shared || d.has_set, a.flags != nullptr, linked_frame});
    // ("debug_shared_dict_items" / "debug_dict_set_items" read the throughput encoder's counters: another encoder has nothing to show)
    if (d.shared) c->shared_counted = enc.mode == 0;
    if (set) c->set_counted = enc.mode == 0 ? set : nullptr;
    if (enc.mode == 2) return compress_high(c, a, d, enc.form, s);
    if (enc.mode == 0) return compress_throughput(c, a, d, s);
    return compress_exact(c, a, d, big, s);
}

// ------------------------------------------------------------------------------------------
// One batch, as every batched entry point and every scalar call describes it.  The pointers are the caller's (host memory for
// run_host_batch, device memory for run_device_batch and launch_batch); what a call does not use stays null / 0.
struct BatchCall {
    bool compress = false;
    const uint8_t* in_base = nullptr;
    const uint64_t* in_off = nullptr;
    const uint32_t* in_len = nullptr;
    const uint32_t* flags = nullptr;        // compress, nullable
    uint32_t n = 0;
    uint8_t* out_base = nullptr;
    const uint64_t* out_off = nullptr;
    const uint32_t* out_cap = nullptr;
    uint32_t* out_len = nullptr;
    int32_t* status = nullptr;
    uint64_t* detail = nullptr;             // decompress, nullable
    const uint8_t* dict_base = nullptr;     // per-block dictionaries (the *_ex calls): all three or none
    const uint64_t* dict_off = nullptr;
    const uint32_t* dict_len = nullptr;
    const uint8_t* shared_dict = nullptr;   // the *_shared_dict calls: ONE dictionary of shared_len bytes for every block (no dict_base then)
    uint32_t shared_len = 0;
    const lz4flex_dict_set* set = nullptr;  // the *_dict_set calls: block i has dictionary dict_id[i] of the set (no dict_base, no shared_dict then)
    const uint32_t* dict_id = nullptr;      // ... in the batch's memory kind
    const uint32_t* out_pos = nullptr;      // decompress: prefix mode
    const uint32_t* chain_prev = nullptr;   // chained DEVICE batches: several chains side by side
    uint32_t n_chains = 0;
    bool has_ext = false;                   // the caller handed an extension struct over, whatever it holds: such a host batch takes the general path
    bool chained = false;                   // LZ4FLEX_MEM_CHAINED
    bool partial = false;                   // the *_partial calls: out_cap holds TARGETS (no detail; with shared_dict or set: the *_partial_shared_dict /
                                            // *_partial_dict_set calls; never with dict_base, a prefix or a chain)
    bool big = false;                       // LZ4FLEX_MEM_BIG_BLOCKS, or -- host batches -- what the lengths say
    bool linked_frame = false;              // compress: the blocks are a Linked frame's (compress_batch_entry: the frame layer says so)
    hipStream_t stream = nullptr;           // DEVICE batches: the caller's (NULL = HIP's null stream); host batches: the context's
};

// the arrays every batch has, in the order the public entry points take them
static BatchCall batch_of(bool compress, const void* in_base, const uint64_t* in_off, const uint32_t* in_len, uint32_t n, void* out_base,
                          const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len, int32_t* status, void* hip_stream = nullptr) {
    BatchCall b;
    b.compress = compress;
    b.in_base = (const uint8_t*)in_base; b.in_off = in_off; b.in_len = in_len; b.n = n;
    b.out_base = (uint8_t*)out_base; b.out_off = out_off; b.out_cap = out_cap; b.out_len = out_len; b.status = status;
    b.stream = (hipStream_t)hip_stream;
    return b;
}

// where the batch's dictionaries come from, either direction (a shared pointer with length 0 is no dictionary: the plain path)
static DictSource dict_source_of(lz4flex_ctx* c, const BatchCall& b) {
    DictSource d{};
    if (b.set) { d.has_set = 1u; d.set = DictSetArgs{b.set->table, b.dict_id, b.set->k, (uint32_t)c->comp_shared, b.set->counter}; }
    else if (b.shared_dict && b.shared_len) { d.shared = b.shared_dict; d.shared_len = b.shared_len; }
    return d;
}

static int launch_encode(lz4flex_ctx* c, const BatchCall& b) {
    CompressArgs a{};
    a.in_base = b.in_base; a.in_off = b.in_off; a.in_len = b.in_len; a.flags = b.flags;
    a.out_base = b.out_base; a.out_off = b.out_off; a.out_cap = b.out_cap; a.out_len = b.out_len; a.status = b.status; a.n = b.n;
    if (b.dict_base) { a.dict_base = b.dict_base; a.dict_off = b.dict_off; a.dict_len = b.dict_len; }
    return launch_compress_any(c, a, dict_source_of(c, b), b.set, b.big, b.linked_frame, b.stream);
}

static int launch_decode(lz4flex_ctx* c, const BatchCall& b) {
    hipStream_t s = b.stream;
    DecompressArgs a{};
    a.in_base = b.in_base; a.in_off = b.in_off; a.in_len = b.in_len;
    a.out_base = b.out_base; a.out_off = b.out_off; a.out_cap = b.out_cap; a.out_pos = b.out_pos;
    a.dict_base = b.dict_base; a.dict_off = b.dict_off; a.dict_len = b.dict_len;
    a.out_len = b.out_len; a.status = b.status; a.detail = b.detail; a.n = b.n;
    const bool chain = b.chained && b.n;
    if (chain) {
        HIP_TRY(chain_ws_begin(c, b.n, s));
        a.chain_done = c->chain_ws;
        a.chain_prev = b.chain_prev;
        a.n_chains = b.n_chains;
        a.debug_giveup = (uint32_t)c->chain_giveup;
    }
    const DictSource d = dict_source_of(c, b);
    if (b.partial) a.detail = nullptr;
    const DecodeRoute r = decode_route(
        DecodeSettings{c->dec_variant, c->dec_pcd_pair, c->dec_shared, c->dec_partial, c->pcd_ws != nullptr, TOOLS_BUILD, plan_fits(b.n)},
        DecodeShape{b.n, b.big, b.out_pos != nullptr, b.chained, b.chain_prev != nullptr, b.n_chains, b.dict_base != nullptr,
                    d.has_set || d.shared != nullptr, b.partial});
    hipError_t le = launch_first_pass(c, a, r, d, b.partial, s);
    if (le == hipSuccess) le = launch_redo(c, a, r.redo, d, b.partial, s);
    if (chain) (void)chain_ws_end(c, s);                     // (also behind a failed launch: whatever was enqueued is ordered)
    return le != hipSuccess ? hip_fail(le, "kernel launch") : 0;
}

static int launch_batch(lz4flex_ctx* c, const BatchCall& b) { return b.compress ? launch_encode(c, b) : launch_decode(c, b); }

extern "C" {

const char* lz4flex_version(void) { return "lz4flex-amd 0.3.0 (gfx950)"; }
#ifndef LZ4FLEX_BUILD_ID
#define LZ4FLEX_BUILD_ID "unstamped"
#endif
const char* lz4flex_build_id(void) { return LZ4FLEX_BUILD_ID; }
const char* lz4flex_last_error(void) { return g_last_error.c_str(); }

int lz4flex_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int lz4flex_ctx_create(lz4flex_ctx** out, int device) {
    if (!out) return -LZ4FLEX_E_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_last_error = "no HIP device available: the MI355X kernels are the only codec in this library";
        return -LZ4FLEX_E_NO_DEVICE;
    }
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    if (device >= n) return -LZ4FLEX_E_INVALID_ARG;
    lz4flex_ctx* c = new (std::nothrow) lz4flex_ctx();
    if (!c) return -LZ4FLEX_E_NOMEM;
    c->device = device;
    c->packed_tile = (int)PACKED_SCAN_TILE;
    if (const char* e = getenv("LZ4FLEX_COMPRESS_MODE")) c->comp_mode = (!strcmp(e, "exact") || !strcmp(e, "1")) ? 1 : (!strcmp(e, "high") || !strcmp(e, "2")) ? 2 : 0;
    if (const char* e = getenv("LZ4FLEX_HIGH_PARSE")) c->comp_parse = (!strcmp(e, "optimal") || !strcmp(e, "1")) ? 1 : 0;
    if (const char* e = getenv("LZ4FLEX_HIGH_DICT")) c->comp_high_dict = !strcmp(e, "1") ? 1 : 0;
    if (const char* e = getenv("LZ4FLEX_HIGH_LINKED")) c->comp_high_linked = !strcmp(e, "1") ? 1 : 0;
    if (const char* e = getenv("LZ4FLEX_SLIDING_WINDOW")) {      // "0", "1" or "2", nothing else ("off" used to read as 0 silently: ADVICE r4)
        if (!strcmp(e, "0") || !strcmp(e, "1") || !strcmp(e, "2")) c->comp_sliding = e[0] - '0';
        else { g_last_error = "LZ4FLEX_SLIDING_WINDOW must be 0, 1 or 2"; delete c; return -LZ4FLEX_E_INVALID_ARG; }
    }
#ifdef LZ4FLEX_ALL_VARIANTS
    if (const char* e = getenv("LZ4FLEX_COMPRESS_VARIANT")) { const int v = atoi(e); if (v == 1 || v == 3) c->comp_variant = v; }
#endif
    if (const char* e = getenv("LZ4FLEX_DECOMPRESS_VARIANT")) { const int v = atoi(e); if (v == 0 || v == 1 || (v >= 4 && v <= 12 && v != 9)) c->dec_variant = v; }
    {
        DeviceGuard guard(device);
        e = guard.err;
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        // the throughput encoder's workspace (two 80 KiB workgroups per CU, 196 MiB on an MI355X with the dictionary staging slots) and its ordering event: here, not
        // inside the first compress call -- a hipMalloc in an "asynchronous" entry point is a device synchronisation and breaks
        // stream capture
        if (e == hipSuccess) {
            int cus = 0;
            e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
            if (e == hipSuccess) {
                c->wave_wgs = 2 * cus;
                e = hipMalloc(&c->wave_ws, compress_wave_workspace_bytes(c->wave_wgs));
            }
        }
        if (e == hipSuccess) e = c->wave.create();
        if (e == hipSuccess) e = hipMalloc((void**)&c->chain_ws, 4u * CHAIN_MAX_BLOCKS);
        if (e == hipSuccess) e = c->chain.create();
        if (e == hipSuccess) e = c->plan.create();
        if (e == hipSuccess) e = c->pcd.create();
        if (e == hipSuccess) e = hipMalloc((void**)&c->pcd_ws, decompress_pcd_pair_ws_bytes());
    }
    if (e != hipSuccess) {
        const int rc = hip_fail(e, "ctx_create");
        lz4flex_ctx_destroy(c);
        return e == hipErrorOutOfMemory ? -LZ4FLEX_E_NOMEM : rc;
    }
    *out = c;
    return 0;
}

void lz4flex_ctx_destroy(lz4flex_ctx* c) {
    if (!c) return;
    c->arena.free();
    if (c->wave_ws) (void)hipFree(c->wave_ws);
    c->wave.destroy();
    if (c->chain_ws) (void)hipFree(c->chain_ws);
    c->chain.destroy();
    if (c->plan_ws) (void)hipFree(c->plan_ws);
    c->plan.destroy();
    if (c->pcd_ws) (void)hipFree(c->pcd_ws);
    c->pcd.destroy();
    if (c->wave_prof) (void)hipFree(c->wave_prof);
    for (void* p : c->many_ws) if (p) (void)hipFree(p);
    c->pin.free();
    c->pay.free();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

#ifdef LZ4FLEX_TOOLS
// variant builds for tools/ only (-DLZ4FLEX_TOOLS; not in the public header, not in the product library): enable != 0 starts /
// resets the wave encoder's per-role cycle counters of this context, vals (nullable) receives the 32 sums accumulated so far
int lz4flex_debug_wave_prof(lz4flex_ctx* c, int enable, unsigned long long* vals) {
    if (!c) return -LZ4FLEX_E_INVALID_ARG;
    if (vals && c->wave_prof) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(vals, c->wave_prof, 256, hipMemcpyDeviceToHost));
    }
    if (enable) {
        if (!c->wave_prof) HIP_TRY(hipMalloc((void**)&c->wave_prof, 256));
        HIP_TRY(hipMemset(c->wave_prof, 0, 256));
    } else if (c->wave_prof) {
        (void)hipFree(c->wave_prof);
        c->wave_prof = nullptr;
    }
    return 0;
}
#endif

}  // extern "C"

// ---- the integer settings: key, field, the values it takes.  lz4flex_set_tuning and lz4flex_get_tuning walk this one table.
namespace {

struct Setting {
    const char* key;
    int lz4flex_ctx::* field;
    bool (*takes)(int value);
    bool set_only;
};
bool is_flag(int v) { return v == 0 || v == 1; }
bool is_count(int v) { return v >= 0; }
bool up_to_2(int v) { return v >= 0 && v <= 2; }
bool read_only(int) { return false; }

const Setting SETTINGS[] = {
    {"decompress_lanes", &lz4flex_ctx::dec_lanes, [](int v) {
#ifdef LZ4FLEX_ALL_VARIANTS
         return v == 8 || v == 16 || v == 32 || v == 64;
#else
         return v == 16;                                        // the other widths exist in variant builds only (-DLZ4FLEX_ALL_VARIANTS)
#endif
     }, false},
    {"compress_mode", &lz4flex_ctx::comp_mode, up_to_2, false},
    {"compress_depth", &lz4flex_ctx::comp_depth, [](int v) { return v >= 1 && v <= 256; }, false},      // "compress_mode" 2: candidates per position
    {"compress_parse", &lz4flex_ctx::comp_parse, is_flag, false},                  // "compress_mode" 2: 0 = the one-step lazy parse, 1 = the optimal one
    {"compress_high_dict", &lz4flex_ctx::comp_high_dict, is_flag, false},          // "compress_mode" 2: dictionary calls take its dictionary form
    {"compress_high_linked", &lz4flex_ctx::comp_high_linked, is_flag, false},      // ... LZ4FLEX_BLOCK_HISTORY bits are read, Linked frames keep the mode
    {"compress_high_digest", &lz4flex_ctx::comp_high_digest, is_flag, false},      // ... and a shared dictionary is sorted once per call
    {"compress_subwindows", &lz4flex_ctx::comp_sub, [](int v) { return v >= 0 && v <= 4; }, false},
    {"compress_deterministic", &lz4flex_ctx::comp_det, is_flag, false},
    {"decompress_level_chains", &lz4flex_ctx::dec_level_chains, is_count, false},
    {"decompress_blocks_per_wg", &lz4flex_ctx::dec_blocks_per_wg, [](int v) { return v == 0 || v == 8 || v == 16 || v == 32 || v == 64; }, false},
    {"decompress_variant", &lz4flex_ctx::dec_variant, [](int v) { return decoder_variant(v, TOOLS_BUILD) != nullptr; }, false},    // lz4_route.h DECODER_VARIANTS
    {"decompress_second_pass", &lz4flex_ctx::dec_second_pass, is_flag, false},
    {"decompress_pcd_pair", &lz4flex_ctx::dec_pcd_pair, up_to_2, false},
    {"compress_carry_wait", &lz4flex_ctx::comp_carry_wait, is_flag, false},
    {"compress_sliding_window", &lz4flex_ctx::comp_sliding, up_to_2, false},
    {"compress_variant", &lz4flex_ctx::comp_variant, [](int v) {
#ifdef LZ4FLEX_ALL_VARIANTS
         return v == 1 || v == 3;
#else
         return v == 1;                                         // 3 (no emitter wavefront) exists in variant builds only
#endif
     }, false},
    {"compress_lanes", &lz4flex_ctx::comp_lanes, [](int v) { return v == 8 || v == 16; }, false},
    {"size_scan_serial", &lz4flex_ctx::size_serial, is_flag, false},
    {"filter_bytewise", &lz4flex_ctx::filter_bytewise, is_flag, false},
    {"fit_serial", &lz4flex_ctx::fit_serial, is_flag, false},
    {"compress_shared_dict", &lz4flex_ctx::comp_shared, is_flag, false},
    {"decompress_shared_dict", &lz4flex_ctx::dec_shared, is_flag, false},
    {"decompress_partial", &lz4flex_ctx::dec_partial, is_flag, false},
    // (frame_index.cpp, lz4flex_frame_read_ranges: the scratch one pass of ranges may take; whether touched blocks' checksums are verified)
    {"frame_range_pass_bytes", &lz4flex_ctx::range_pass_bytes, [](int v) { return v >= 1; }, false},
    {"frame_range_checksums", &lz4flex_ctx::range_checksums, is_flag, false},
    // (the sizes one workgroup of the packed entries' offset scan takes: lz4_device.h PACKED_SCAN_TILE; the tests cut their batches around it)
    {"packed_scan_tile", &lz4flex_ctx::packed_tile, read_only, false},
    // (what "compress_subwindows" 0 decides by: n * 4 <= this -> 4, n * 3 <= this -> 3, n * 2 <= this -> 2)
    {"compress_workgroups", &lz4flex_ctx::wave_wgs, read_only, false},
    {"debug_chain_giveup", &lz4flex_ctx::chain_giveup, is_count, true},
    {"debug_exact_dict_piece", &lz4flex_ctx::exact_dict_piece, is_count, true},    // tests/test_gpu_exact_dict_pieces.py: more than one piece
    {"debug_fail_next_batch", &lz4flex_ctx::fail_next_batch, is_count, true},      // tests/test_gpu_sharded_native.py: one rank's call-level failure
    {"debug_fit_first_pass", &lz4flex_ctx::fit_first_pass, is_flag, true},         // tests/test_gpu_fit.py: which blocks does the wavefront pass finish?
};
const Setting* find_setting(const char* key) {
    for (const Setting& s : SETTINGS) if (!strcmp(key, s.key)) return &s;
    return nullptr;
}

// Test hooks (every "debug_" key; fault injection, unsupported, see the header): only in a process that opted in with LZ4FLEX_TEST_HOOKS=1
// (tests/conftest.py does) -- the frame layer and every scalar call of a process share the default context, a hook set there by anybody
// else would make unrelated users fail or take the slow redo path.  Refused before a context is looked for.
bool key_allowed(const char* key) {
    if (strncmp(key, "debug_", 6) != 0) return true;
    const char* e = getenv("LZ4FLEX_TEST_HOOKS");
    return e && !strcmp(e, "1");
}

// "<prefix><i>": the i of a list that ends where the key is refused (-1: not a number)
int list_index(const char* index) { return index[0] < '0' || index[0] > '9' ? -1 : atoi(index); }

// "debug_shared_dict_items": the items of the last lz4flex_compress_batch_shared_dict call on this context whose first window started
// from the digest (0: none yet, the reference-exact mode, "compress_shared_dict" 0); waits for the device
int shared_dict_items(lz4flex_ctx* c) {
    if (!c->shared_counted || !c->wave_ws) return 0;
    DeviceGuard guard(c->device);
    HIP_TRY(guard.err);
    uint32_t v = 0;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(&v, compress_wave_shared_counter(c->wave_ws, c->wave_wgs), 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "debug_shared_dict_items");
    return (int)std::min<uint32_t>(v, 0x7FFFFFFFu);
}

// "debug_dict_set_items": the same for the last lz4flex_compress_batch_dict_set call on this context, read from that call's set (0: none
// yet, the reference-exact mode, "compress_shared_dict" 0, a set that has been freed since)
int dict_set_items(lz4flex_ctx* c) {
    std::lock_guard<std::mutex> lock(g_sets_mu);
    if (!c->set_counted || std::find(g_live_sets.begin(), g_live_sets.end(), c->set_counted) == g_live_sets.end()) return 0;
    DeviceGuard guard(c->device);
    HIP_TRY(guard.err);
    uint32_t v = 0;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(&v, c->set_counted->counter, 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "debug_dict_set_items");
    return (int)std::min<uint32_t>(v, 0x7FFFFFFFu);
}

}  // namespace

extern "C" {

int lz4flex_set_tuning(lz4flex_ctx* c, const char* key, int value) {
    if (!key) return -LZ4FLEX_E_INVALID_ARG;
    const Setting* st = find_setting(key);
    if (!st || !key_allowed(key)) return -LZ4FLEX_E_INVALID_ARG;
    if (!c) { const int rc = default_ctx(&c); if (rc) return rc; }   // NULL: this thread's default context (the scalar calls)
    if (!st->takes(value)) return -LZ4FLEX_E_INVALID_ARG;
    c->*(st->field) = value;
    return 0;
}

int lz4flex_get_tuning(lz4flex_ctx* c, const char* key) {
    if (!key) return -LZ4FLEX_E_INVALID_ARG;
    // the batch sizes at which the default decoder dispatch changes kernel or geometry (lz4_route.h DISPATCH_THRESHOLDS), in ascending
    // order; the list ends where the key is refused.  tests/test_gpu_block.py builds its size matrix from it.
    if (!strncmp(key, "dispatch_threshold_", 19)) {
        const int i = list_index(key + 19);
        return i >= 0 && i < (int)(sizeof DISPATCH_THRESHOLDS / sizeof DISPATCH_THRESHOLDS[0]) ? (int)DISPATCH_THRESHOLDS[i] : -LZ4FLEX_E_INVALID_ARG;
    }
    // every decoder configuration this build can be pinned to, as variant * 1000 + parameter ("decompress_lanes" for variant 1,
    // "decompress_blocks_per_wg" for variant 4, else 0); the list ends where the key is refused.  ONE list, read off lz4_route.h
    // DECODER_VARIANTS: tests/test_gpu_block.py's decoder matrix and tools/gpu_fuzz.py are generated from it (a decoder added to the
    // table is tested there), no device needed.
    if (!strncmp(key, "decoder_config_", 15)) {
        const int v = decoder_config(list_index(key + 15), TOOLS_BUILD);
        return v >= 0 ? v : -LZ4FLEX_E_INVALID_ARG;
    }
    const bool set_items = !strcmp(key, "debug_dict_set_items");
    const bool items = set_items || !strcmp(key, "debug_shared_dict_items");
    const Setting* st = items ? nullptr : find_setting(key);
    if ((!items && !st) || !key_allowed(key)) return -LZ4FLEX_E_INVALID_ARG;
    if (!c) { const int rc = default_ctx(&c); if (rc) return rc; }
    if (items) return set_items ? dict_set_items(c) : shared_dict_items(c);
    return st->set_only ? -LZ4FLEX_E_INVALID_ARG : c->*(st->field);
}

int lz4flex_abi_version(void) { return 8; }

size_t lz4flex_get_maximum_output_size(size_t input_len) {
    return 16 + 4 + (size_t)((uint64_t)input_len * 110 / 100);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// host-resident batches: mirror the caller's layout in the device arena, run, copy back
namespace {

// the bytes [lo, hi) that (offset, length) pairs cover; nothing added (or lengths that wrap): empty at 0
struct Span {
    uint64_t lo = ~0ull, hi = 0;
    void add(uint64_t off, uint64_t len) { lo = std::min<uint64_t>(lo, off); hi = std::max<uint64_t>(hi, off + len); }
    Span closed() const { return lo > hi ? Span{0, 0} : *this; }
    size_t bytes() const { return (size_t)(hi - lo); }
};
Span span_of(const uint64_t* off, const uint32_t* len, uint32_t n) {
    Span s;
    for (uint32_t i = 0; i < n; i++) s.add(off[i], len[i]);
    return s.closed();
}

// host arrays are visible: a batch with a block beyond 64 KiB (compress) / 128 KiB compressed (decompress) is one of "large" blocks
bool host_big(const uint32_t* len, uint32_t n, bool compress) {
    const uint32_t limit = compress ? 65536u : 131072u;
    bool big = false;
    for (uint32_t i = 0; i < n; i++) big |= len[i] > limit;
    return big;
}

// a codec call's fetched result columns to the caller's arrays (detail: what a decoder reports, zero for compress)
void copy_results(const BatchCall& b, const uint32_t* r_len, const int32_t* r_st, const uint64_t* r_det) {
    memcpy(b.out_len, r_len, 4ull * b.n);
    memcpy(b.status, r_st, 4ull * b.n);
    if (!b.detail) return;
    if (b.compress) memset(b.detail, 0, 16ull * b.n);
    else memcpy(b.detail, r_det, 16ull * b.n);
}

// every block with status 0 (st null: every block) and a length goes from page-locked memory -- src_off(i) of `src` -- to its place in
// the caller's buffer; nothing else of that buffer is written: a failed block and the gaps between blocks stay the caller's.  limit: the
// bytes `src` holds, a block that ends behind them is left alone too
template <class SrcOff>
void scatter_good(uint8_t* out_base, const uint64_t* out_off, const uint32_t* len, const int32_t* st, uint32_t n, const uint8_t* src, SrcOff src_off,
                  uint64_t limit = ~0ull) {
    for (uint32_t i = 0; i < n; i++)
        if ((!st || st[i] == 0) && len[i] && (uint64_t)src_off(i) + len[i] <= limit) memcpy(out_base + out_off[i], src + src_off(i), len[i]);
}

}  // namespace

// A host batch of a few small blocks (the scalar calls above all: compress_into / decompress_into are 1-block batches): ONE transfer up
// (descriptors + input, from page-locked staging), the kernels, ONE transfer down (results + output), one synchronisation -- the
// general path below costs two transfers each way from pageable memory and two synchronisations (0.16 / 0.38 ms per 64 KiB block in
// round 3).  Same semantics: a block that failed leaves the caller's bytes alone.  For batches without dictionaries, prefixes or a
// chain only: run_host_batch sees to that.  The input blocks and the output slots are columns of the image here (64-byte starts, a slot
// per block), and the image is the arena's one region.
static constexpr uint32_t SMALL_BATCH_BLOCKS = 8u;
static constexpr size_t SMALL_BATCH_BYTES = 4u << 20;
static int run_host_small(lz4flex_ctx* c, const BatchCall& b) {
    const uint32_t n = b.n;
    auto in_slot = [&](uint32_t i) { return align_up(b.in_len[i] + 16, 64); };
    auto out_slot = [&](uint32_t i) { return align_up((size_t)b.out_cap[i] + 16, 64); };
    size_t in_bytes = 0, out_bytes = 0;
    for (uint32_t i = 0; i < n; i++) { in_bytes += in_slot(i); out_bytes += out_slot(i); }
    HostStage st(64);
    const auto in_off = st.up<uint64_t>(n), out_off = st.up<uint64_t>(n);
    const auto in_len = st.up<uint32_t>(n), out_cap = st.up<uint32_t>(n), flags = st.up<uint32_t>(n);
    const auto in = st.up<uint8_t>(in_bytes);
    const auto out_len = st.down<uint32_t>(n);
    const auto status = st.down<int32_t>(n);
    const auto detail = st.down<uint64_t>(2ull * n);
    const auto out = st.down<uint8_t>(out_bytes);
    st.columns();
    int rc;
    if ((rc = stage_open(c, st))) return rc;
    uint64_t *const in_at = st.host(in_off), *const out_at = st.host(out_off);
    size_t ia = 0, oa = 0;
    for (uint32_t i = 0; i < n; i++) {
        in_at[i] = ia;
        out_at[i] = oa;
        if (b.in_len[i]) memcpy(st.host(in) + ia, b.in_base + b.in_off[i], b.in_len[i]);
        ia += in_slot(i);
        oa += out_slot(i);
    }
    st.fill(in_len, b.in_len); st.fill(out_cap, b.out_cap);
    if (b.flags) st.fill(flags, b.flags); else st.zero(flags);
    HIP_TRY(st.send_columns());
    // the batch as it lies in the arena
    BatchCall dv = batch_of(b.compress, st.dev(in), st.dev(in_off), st.dev(in_len), n, st.dev(out), st.dev(out_off), st.dev(out_cap), st.dev(out_len),
                            st.dev(status), st.s);
    dv.big = host_big(b.in_len, n, b.compress); dv.partial = b.partial; dv.linked_frame = b.linked_frame;
    dv.flags = b.flags ? st.dev(flags) : nullptr;
    dv.detail = st.dev(detail);
    if ((rc = launch_batch(c, dv))) return rc;
    HIP_TRY(st.fetch_columns(out_len));
    HIP_TRY(hipStreamSynchronize(st.s));
    copy_results(b, st.host(out_len), st.host(status), st.host(detail));
    scatter_good(b.out_base, b.out_off, st.host(out_len), st.host(status), n, st.host(out), [&](uint32_t i) { return out_at[i]; });
    return 0;
}

static int run_host_batch(lz4flex_ctx* c, const BatchCall& b) {
    const uint32_t n = b.n;
    if (n == 0) return 0;
    if (b.chained && (n > CHAIN_MAX_BLOCKS || !b.out_pos || b.dict_base)) return -LZ4FLEX_E_INVALID_ARG;
    if (b.chain_prev) return -LZ4FLEX_E_INVALID_ARG;                // several chains in one batch: DEVICE batches only (a host batch stages ONE output region)
    DeviceGuard guard(c->device);
    HIP_TRY(guard.err);
    // LZ4FLEX_BLOCK_HISTORY: the bytes in front of a block travel with it
    uint64_t hist_lo = ~0ull;
    if (b.compress && b.flags)
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t h = b.flags[i] >> 8;
            if (h > b.in_off[i]) return -LZ4FLEX_E_INVALID_ARG;
            if (h) hist_lo = std::min<uint64_t>(hist_lo, b.in_off[i] - h);
        }
    const bool has_dict = b.dict_base && b.dict_off && b.dict_len;
    const bool has_pos = b.out_pos != nullptr;
    const bool has_shared = b.shared_dict && b.shared_len;
    if (n <= SMALL_BATCH_BLOCKS && !b.has_ext && !b.chained && hist_lo == ~0ull) {
        size_t bytes = 0;
        for (uint32_t i = 0; i < n; i++) bytes += (size_t)b.in_len[i] + b.out_cap[i];
        if (bytes <= SMALL_BATCH_BYTES) return run_host_small(c, b);
    }

    Span in_span = span_of(b.in_off, b.in_len, n), dict_span;
    if (hist_lo < in_span.lo) in_span.lo = hist_lo;
    const Span out_span = span_of(b.out_off, b.out_cap, n);
    if (has_dict) {
        // (compress: the dictionary offsets of blocks without one are not looked at -- they need not lie anywhere near the others)
        for (uint32_t i = 0; i < n; i++)
            if (!b.compress || b.dict_len[i]) dict_span.add(b.dict_off[i], b.dict_len[i]);
        dict_span = dict_span.closed();
    }
    const size_t out_bytes = out_span.bytes();
    HostStage st;
    const auto in_off = st.up<uint64_t>(n), out_off = st.up<uint64_t>(n), dict_off = st.up<uint64_t>(has_dict ? n : 0);
    const auto in_len = st.up<uint32_t>(n), out_cap = st.up<uint32_t>(n), flags = st.up<uint32_t>(b.flags ? n : 0),
               dict_len = st.up<uint32_t>(has_dict ? n : 0), out_pos = st.up<uint32_t>(has_pos ? n : 0), dict_id = st.up<uint32_t>(b.set ? n : 0);
    const auto out_len = st.down<uint32_t>(n);
    const auto status = st.down<int32_t>(n);
    const auto detail = st.down<uint64_t>(2ull * n);
    const Region r_in = st.region(in_span.bytes(), 64), r_out = st.region(out_bytes, 64),
                 r_dict = st.region(has_shared ? (size_t)b.shared_len : has_dict ? dict_span.bytes() : 0, 64);
    st.columns();
    int rc;
    if ((rc = stage_open(c, st))) return rc;
    st.fill_offsets(in_off, b.in_off, in_span.lo); st.fill_offsets(out_off, b.out_off, out_span.lo);
    st.fill_offsets(dict_off, b.dict_off, dict_span.lo, b.compress ? b.dict_len : nullptr);
    st.fill(in_len, b.in_len); st.fill(out_cap, b.out_cap); st.fill(flags, b.flags); st.fill(dict_len, b.dict_len); st.fill(out_pos, b.out_pos);
    st.fill(dict_id, b.dict_id);                                  // (the ids travel with the batch; the dictionaries are on the device already)
    hipStream_t s = st.s;
    HIP_TRY(st.send(r_in, b.in_base + in_span.lo));
    HIP_TRY(st.send(r_dict, has_shared ? b.shared_dict : has_dict ? b.dict_base + dict_span.lo : nullptr));
    if (has_pos && out_bytes) {
        // prefix mode: the sink already holds bytes [0, out_pos) that matches may reference; in a chained batch only what lies
        // before the FIRST block's position exists yet (the rest is what the batch produces)
        const size_t up = b.chained ? std::min<size_t>(out_bytes, (size_t)(b.out_off[0] - out_span.lo) + b.out_pos[0]) : out_bytes;
        HIP_TRY(st.send(r_out, b.out_base + out_span.lo, up));
    }
    HIP_TRY(st.send_columns());
    // the batch as it lies in the arena
    BatchCall dv = batch_of(b.compress, st.dev(r_in), st.dev(in_off), st.dev(in_len), n, st.dev(r_out), st.dev(out_off), st.dev(out_cap),
                            st.dev(out_len), st.dev(status), s);
    dv.chained = b.chained; dv.big = host_big(b.in_len, n, b.compress); dv.partial = b.partial; dv.linked_frame = b.linked_frame;
    dv.flags = st.dev_opt(flags);
    dv.detail = st.dev(detail);
    if (has_dict) { dv.dict_base = st.dev(r_dict); dv.dict_off = st.dev(dict_off); dv.dict_len = st.dev(dict_len); }
    if (has_shared) { dv.shared_dict = st.dev(r_dict); dv.shared_len = b.shared_len; }
    dv.out_pos = st.dev_opt(out_pos);
    if (b.set) { dv.set = b.set; dv.dict_id = st.dev(dict_id); }
    if ((rc = launch_batch(c, dv))) return rc;
    HIP_TRY(st.fetch_columns(out_len));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t* r_len = st.host(out_len);
    const int32_t* r_st = st.host(status);
    copy_results(b, r_len, r_st, st.host(detail));
    uint64_t produced = 0;
    for (uint32_t i = 0; i < n; i++)
        if (r_st[i] == 0) produced += r_len[i];
    uint8_t* const d_out = st.dev(r_out);
    // copy results back: dense outputs in one transfer, sparse ones block by block
    if (out_bytes && produced * 2 >= out_bytes && !has_pos) {
        // every successful block owns [out_off, out_off+len); failed blocks must leave the caller's bytes alone
        // ... and the one-shot copy covers the whole span, so the blocks must TILE it: with gaps between the callers' slots (a
        // padded stride) it would overwrite host bytes that belong to nobody with whatever the device arena holds
        // (round 6: the block that ENDS the span may be short -- a frame's last block, lz4flex_frame_decompress decoding straight into the
        // caller's buffer -- the transfer then stops at its last byte)
        bool all_ok = true;
        uint64_t cap_sum = 0, short_tail = 0;
        for (uint32_t i = 0; i < n; i++) {
            cap_sum += b.out_cap[i];
            if (r_st[i] != 0) { all_ok = false; break; }
            if (r_len[i] == b.out_cap[i]) continue;
            if (b.out_off[i] + b.out_cap[i] == out_span.hi && short_tail == 0 && r_len[i] < b.out_cap[i]) short_tail = b.out_cap[i] - r_len[i];
            else { all_ok = false; break; }
        }
        all_ok = all_ok && cap_sum == (uint64_t)out_bytes;
        if (all_ok) {
            if (out_bytes > short_tail) HIP_TRY(hipMemcpyAsync(b.out_base + out_span.lo, d_out, out_bytes - (size_t)short_tail, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            return 0;
        }
    }
    // sparse results, many blocks: pack them on the device into the (now free) input region, one transfer to pinned
    // memory, scatter on the host.  A per-block hipMemcpy to pageable memory costs ~10 us each.
    if (!has_pos && n >= 16u && produced != 0 && produced <= (uint64_t)r_in.room && ensure_buf(c->pay, (size_t)produced) == 0) {
        uint64_t* h_dense = st.host(detail);                      // reuse the detail slot (16 B per block >= 8 B)
        uint64_t at = 0;
        for (uint32_t i = 0; i < n; i++) { h_dense[i] = at; if (r_st[i] == 0) at += r_len[i]; }
        HIP_TRY(hipMemcpyAsync(st.dev(detail), h_dense, 8ull * n, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(lz4flex_pack_results_kernel, dim3(n), dim3(256), 0, s, d_out, st.dev(out_off), st.dev(out_len), st.dev(status),
                           st.dev(detail), st.dev(r_in), n);
        const hipError_t pe = hipGetLastError();              // (reading it clears it: read once)
        if (pe != hipSuccess) return hip_fail(pe, "pack kernel launch");
        HIP_TRY(hipMemcpyAsync(c->pay.p, st.dev(r_in), (size_t)produced, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        scatter_good(b.out_base, b.out_off, r_len, r_st, n, c->pay.p, [&](uint32_t i) { return h_dense[i]; });
        return 0;
    }
    if (b.chained) {
        // one region, the blocks back to back behind the first one's position: one transfer up to the end of the last good block
        uint64_t lo = b.out_off[0] + b.out_pos[0], hi = lo;
        for (uint32_t i = 0; i < n; i++)
            if (r_st[i] == 0) hi = std::max<uint64_t>(hi, b.out_off[i] + b.out_pos[i] + r_len[i]);
        if (hi > lo) HIP_TRY(hipMemcpyAsync(b.out_base + lo, d_out + (lo - out_span.lo), (size_t)(hi - lo), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return 0;
    }
    for (uint32_t i = 0; i < n; i++) {
        if (r_st[i] != 0 || r_len[i] == 0) continue;
        const uint32_t pos = has_pos ? b.out_pos[i] : 0u;
        HIP_TRY(hipMemcpyAsync(b.out_base + b.out_off[i] + pos, d_out + (b.out_off[i] - out_span.lo) + pos, r_len[i], hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// DEVICE batches run on the caller's stream, on the caller's arrays
static int run_device_batch(lz4flex_ctx* c, const BatchCall& b) {
    if (b.chained ? (b.compress || b.n > CHAIN_MAX_BLOCKS || !b.out_pos || b.dict_base) : b.chain_prev != nullptr) return -LZ4FLEX_E_INVALID_ARG;
    return launch_batch(c, b);
}

// frame_many.cpp's view of a context (lz4_ctx.h): the context or the calling thread's default one; grow-only scratch
namespace lz4flex_dev {
int ctx_resolve(lz4flex_ctx** ctx) { return *ctx ? 0 : default_ctx(ctx); }
int ctx_scratch(lz4flex_ctx* c, int slot, size_t bytes, void** out) {
    if (slot < 0 || slot >= 4) return -LZ4FLEX_E_INVALID_ARG;
    if (bytes > c->many_cap[slot]) {
        if (c->many_ws[slot]) (void)hipFree(c->many_ws[slot]);
        c->many_ws[slot] = nullptr; c->many_cap[slot] = 0;
        const size_t want = bytes + bytes / 8 + 4096;
        const hipError_t e = hipMalloc(&c->many_ws[slot], want);
        if (e != hipSuccess) { (void)hip_fail(e, "scratch"); return e == hipErrorOutOfMemory ? -LZ4FLEX_E_NOMEM : -LZ4FLEX_E_HIP; }
        c->many_cap[slot] = want;
    }
    *out = c->many_ws[slot];
    return 0;
}
}  // namespace lz4flex_dev

// ---- what the batched entry points share.  Each keeps ITS order of checks and ITS accepted mem_kind values: both are observable.
namespace {

bool batch_arrays_ok(const BatchCall& b) {
    return !b.n || (b.in_off && b.in_len && b.out_off && b.out_cap && b.out_len && b.status);
}

// "debug_fail_next_batch" (tests)
int injected_failure(lz4flex_ctx* c) {
    if (c->fail_next_batch <= 0) return 0;
    c->fail_next_batch--;
    g_last_error = "debug_fail_next_batch";
    return -LZ4FLEX_E_HIP;
}
// the entry points that check their arguments first (a wrong call says so on any machine): then the context, then the hook
int begin_batch(lz4flex_ctx** ctx) {
    const int rc = ctx_resolve(ctx);
    return rc ? rc : injected_failure(*ctx);
}

// mem_kind: the low byte says where the buffers are, the bits above it are flags.  An entry point accepts HOST with the flags of
// host_flags at most and DEVICE with those of device_flags at most.
enum class Mem { Host, Device, Invalid };
struct MemKind { Mem where; bool big, chained; };
constexpr int ANY_FLAGS = ~0xFF;
MemKind classify_mem(int mem_kind, int host_flags, int device_flags) {
    const int where = mem_kind & 0xFF, flags = mem_kind & ~0xFF;
    MemKind k{Mem::Invalid, (flags & LZ4FLEX_MEM_BIG_BLOCKS) != 0, (flags & LZ4FLEX_MEM_CHAINED) != 0};
    if (where == LZ4FLEX_MEM_HOST && !(flags & ~host_flags)) k.where = Mem::Host;
    if (where == LZ4FLEX_MEM_DEVICE && !(flags & ~device_flags)) k.where = Mem::Device;
    return k;
}

int run_batch(lz4flex_ctx* c, BatchCall& b, const MemKind& k) {
    if (k.where == Mem::Invalid) return -LZ4FLEX_E_INVALID_ARG;
    b.big = k.big;
    return k.where == Mem::Host ? run_host_batch(c, b) : run_device_batch(c, b);
}

}  // namespace

// lz4_batch_entry.h: lz4flex_compress_batch, and what the frame layer calls for a Linked frame's blocks
int lz4flex_dev::compress_batch_entry(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len, const uint32_t* flags,
                                      uint32_t n, void* out_base, const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len, int32_t* status,
                                      int mem_kind, void* hip_stream, bool linked_frame) {
    int rc;
    if ((rc = ctx_resolve(&ctx))) return rc;
    BatchCall b = batch_of(true, in_base, in_off, in_len, n, out_base, out_off, out_cap, out_len, status, hip_stream);
    b.flags = flags; b.linked_frame = linked_frame;
    if (!batch_arrays_ok(b)) return -LZ4FLEX_E_INVALID_ARG;
    if ((rc = injected_failure(ctx))) return rc;
    return run_batch(ctx, b, classify_mem(mem_kind, 0, ANY_FLAGS));      // (of the flags, DEVICE batches read BIG_BLOCKS alone)
}

extern "C" {

int lz4flex_compress_batch(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len,
                           const uint32_t* flags, uint32_t n, void* out_base, const uint64_t* out_off,
                           const uint32_t* out_cap, uint32_t* out_len, int32_t* status, int mem_kind,
                           void* hip_stream) {
    return compress_batch_entry(ctx, in_base, in_off, in_len, flags, n, out_base, out_off, out_cap, out_len, status, mem_kind, hip_stream, false);
}

int lz4flex_compress_batch_ex(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len,
                              const uint32_t* flags, uint32_t n, void* out_base, const uint64_t* out_off,
                              const uint32_t* out_cap, uint32_t* out_len, int32_t* status,
                              const lz4flex_compress_ext* ext, int mem_kind, void* hip_stream) {
    if (!ext || !ext->dict_base)
        return lz4flex_compress_batch(ctx, in_base, in_off, in_len, flags, n, out_base, out_off, out_cap, out_len, status, mem_kind, hip_stream);
    if (!ext->dict_off || !ext->dict_len) return -LZ4FLEX_E_INVALID_ARG;
    BatchCall b = batch_of(true, in_base, in_off, in_len, n, out_base, out_off, out_cap, out_len, status, hip_stream);
    b.flags = flags;
    b.has_ext = true; b.dict_base = (const uint8_t*)ext->dict_base; b.dict_off = ext->dict_off; b.dict_len = ext->dict_len;
    if (!batch_arrays_ok(b)) return -LZ4FLEX_E_INVALID_ARG;
    const MemKind k = classify_mem(mem_kind, 0, LZ4FLEX_MEM_BIG_BLOCKS);
    if (k.where == Mem::Invalid) return -LZ4FLEX_E_INVALID_ARG;
    const int rc = begin_batch(&ctx);
    return rc ? rc : run_batch(ctx, b, k);
}

int lz4flex_compress_batch_shared_dict(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len,
                                       uint32_t n, void* out_base, const uint64_t* out_off, const uint32_t* out_cap,
                                       uint32_t* out_len, int32_t* status, const void* dict, uint32_t dict_len,
                                       int mem_kind, void* hip_stream) {
    if (!dict && dict_len) return -LZ4FLEX_E_INVALID_ARG;
    BatchCall b = batch_of(true, in_base, in_off, in_len, n, out_base, out_off, out_cap, out_len, status, hip_stream);
    b.has_ext = true; b.shared_dict = (const uint8_t*)dict; b.shared_len = dict_len;
    if (!batch_arrays_ok(b)) return -LZ4FLEX_E_INVALID_ARG;
    const MemKind k = classify_mem(mem_kind, 0, LZ4FLEX_MEM_BIG_BLOCKS);
    if (k.where == Mem::Invalid) return -LZ4FLEX_E_INVALID_ARG;
    // "debug_shared_dict_items" speaks of THIS call from here on: one that forwards or has nothing to do counts nothing
    if (lz4flex_ctx* c0 = ctx ? ctx : g_default_ctx) c0->shared_counted = false;
    if (n == 0) return 0;
    if (!dict || !dict_len)
        return lz4flex_compress_batch(ctx, in_base, in_off, in_len, nullptr, n, out_base, out_off, out_cap, out_len, status, mem_kind, hip_stream);
    const int rc = begin_batch(&ctx);
    return rc ? rc : run_batch(ctx, b, k);
}

int lz4flex_decompress_batch_ex(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len,
                                uint32_t n, void* out_base, const uint64_t* out_off, const uint32_t* out_cap,
                                uint32_t* out_len, int32_t* status, uint64_t* detail,
                                const lz4flex_decompress_ext* ext, int mem_kind, void* hip_stream) {
    int rc;
    if ((rc = ctx_resolve(&ctx))) return rc;
    BatchCall b = batch_of(false, in_base, in_off, in_len, n, out_base, out_off, out_cap, out_len, status, hip_stream);
    b.detail = detail;
    if (!batch_arrays_ok(b)) return -LZ4FLEX_E_INVALID_ARG;
    if ((rc = injected_failure(ctx))) return rc;
    const MemKind k = classify_mem(mem_kind, ANY_FLAGS, ANY_FLAGS);
    b.chained = k.chained;
    if (ext) {
        b.has_ext = true;
        b.dict_base = (const uint8_t*)ext->dict_base; b.dict_off = ext->dict_off; b.dict_len = ext->dict_len; b.out_pos = ext->out_pos;
        // chain_prev / n_chains (round 5) lie behind the four members every earlier caller knows: they are only looked at in the one
        // batch shape that uses them -- a caller built against the round-4 header hands over a 32-byte struct (lz4flex_abi_version)
        if (k.chained && k.where == Mem::Device) { b.chain_prev = ext->chain_prev; b.n_chains = ext->n_chains; }
    }
    return run_batch(ctx, b, k);
}

int lz4flex_decompress_batch_shared_dict(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len,
                                         uint32_t n, void* out_base, const uint64_t* out_off, const uint32_t* out_cap,
                                         uint32_t* out_len, int32_t* status, uint64_t* detail, const void* dict, uint32_t dict_len,
                                         int mem_kind, void* hip_stream) {
    if (!dict && dict_len) return -LZ4FLEX_E_INVALID_ARG;
    BatchCall b = batch_of(false, in_base, in_off, in_len, n, out_base, out_off, out_cap, out_len, status, hip_stream);
    b.detail = detail; b.has_ext = true; b.shared_dict = (const uint8_t*)dict; b.shared_len = dict_len;
    if (!batch_arrays_ok(b)) return -LZ4FLEX_E_INVALID_ARG;
    const MemKind k = classify_mem(mem_kind, LZ4FLEX_MEM_BIG_BLOCKS, LZ4FLEX_MEM_BIG_BLOCKS);     // (no LZ4FLEX_MEM_CHAINED)
    if (k.where == Mem::Invalid) return -LZ4FLEX_E_INVALID_ARG;
    if (n == 0) return 0;
    if (!dict || !dict_len)
        return lz4flex_decompress_batch(ctx, in_base, in_off, in_len, n, out_base, out_off, out_cap, out_len, status, detail, mem_kind, hip_stream);
    const int rc = begin_batch(&ctx);
    return rc ? rc : run_batch(ctx, b, k);
}

int lz4flex_decompress_batch_partial(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len, uint32_t n,
                                     void* out_base, const uint64_t* out_off, const uint32_t* target, uint32_t* out_len, int32_t* status,
                                     int mem_kind, void* hip_stream) {
    BatchCall b = batch_of(false, in_base, in_off, in_len, n, out_base, out_off, target, out_len, status, hip_stream);
    b.partial = true;
    if (!batch_arrays_ok(b)) return -LZ4FLEX_E_INVALID_ARG;
    const MemKind k = classify_mem(mem_kind, LZ4FLEX_MEM_BIG_BLOCKS, LZ4FLEX_MEM_BIG_BLOCKS);     // (no LZ4FLEX_MEM_CHAINED)
    if (k.where == Mem::Invalid) return -LZ4FLEX_E_INVALID_ARG;
    if (n == 0) return 0;
    const int rc = begin_batch(&ctx);
    return rc ? rc : run_batch(ctx, b, k);
}

int lz4flex_decompress_batch_partial_shared_dict(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len, uint32_t n,
                                                 void* out_base, const uint64_t* out_off, const uint32_t* target, uint32_t* out_len, int32_t* status,
                                                 const void* dict, uint32_t dict_len, int mem_kind, void* hip_stream) {
    if (!dict && dict_len) return -LZ4FLEX_E_INVALID_ARG;
    BatchCall b = batch_of(false, in_base, in_off, in_len, n, out_base, out_off, target, out_len, status, hip_stream);
    b.partial = true; b.has_ext = true; b.shared_dict = (const uint8_t*)dict; b.shared_len = dict_len;
    if (!batch_arrays_ok(b)) return -LZ4FLEX_E_INVALID_ARG;
    const MemKind k = classify_mem(mem_kind, LZ4FLEX_MEM_BIG_BLOCKS, LZ4FLEX_MEM_BIG_BLOCKS);     // (no LZ4FLEX_MEM_CHAINED)
    if (k.where == Mem::Invalid) return -LZ4FLEX_E_INVALID_ARG;
    if (n == 0) return 0;
    if (!dict || !dict_len)
        return lz4flex_decompress_batch_partial(ctx, in_base, in_off, in_len, n, out_base, out_off, target, out_len, status, mem_kind, hip_stream);
    const int rc = begin_batch(&ctx);
    return rc ? rc : run_batch(ctx, b, k);
}

// ---- dictionary sets ----------------------------------------------------------------------------------------------------------
int lz4flex_dict_set_create(lz4flex_ctx* ctx, const void* dict_base, const uint64_t* dict_off, const uint32_t* dict_len, uint32_t k,
                            int mem_kind, lz4flex_dict_set** out) {
    if (out) *out = nullptr;
    if (!out || !dict_off || !dict_len || k == 0u || k > DICT_SET_MAX) return -LZ4FLEX_E_INVALID_ARG;
    if (mem_kind != LZ4FLEX_MEM_HOST && mem_kind != LZ4FLEX_MEM_DEVICE) return -LZ4FLEX_E_INVALID_ARG;
    int rc;
    if ((rc = ctx_resolve(&ctx))) return rc;
    DeviceGuard guard(ctx->device);
    HIP_TRY(guard.err);
    // a DEVICE caller's descriptor arrays are device memory: their host copy
    std::vector<uint64_t> offs(k);
    std::vector<uint32_t> lens(k);
    const hipMemcpyKind from = mem_kind == LZ4FLEX_MEM_DEVICE ? hipMemcpyDeviceToHost : hipMemcpyHostToHost;
    HIP_TRY(hipMemcpy(offs.data(), dict_off, 8ull * k, from));
    HIP_TRY(hipMemcpy(lens.data(), dict_len, 4ull * k, from));
    // [table | counter | a digest per dictionary | the kept bytes, each dictionary's start 256-byte aligned]
    const size_t dg = compress_wave_digest_bytes();
    Layout l{256};
    const size_t at_table = l.take(sizeof(DictSetRec) * (size_t)k), at_counter = l.take(4), at_digest = l.take(dg * k);
    std::vector<size_t> at_bytes(k);
    bool any = false;
    for (uint32_t d = 0; d < k; d++) {
        at_bytes[d] = l.take(std::min<uint32_t>(lens[d], DICT_KEEP));
        any |= lens[d] != 0u;
    }
    if (any && !dict_base) return -LZ4FLEX_E_INVALID_ARG;
    lz4flex_dict_set* set = new (std::nothrow) lz4flex_dict_set();
    if (!set) return -LZ4FLEX_E_NOMEM;
    set->device = ctx->device; set->k = k;
    uint8_t* scratch = nullptr;
    hipStream_t s = ctx->stream;
    hipError_t e = hipMalloc((void**)&set->mem, l.end + 256);
    if (e == hipSuccess) e = hipMalloc((void**)&scratch, compress_wave_digest_scratch_bytes() * k);
    std::vector<DictSetRec> table(k);
    for (uint32_t d = 0; d < k && e == hipSuccess; d++) {
        DictSetRec& r = table[d];
        r.len = lens[d];
        r.kept = std::min<uint32_t>(lens[d], DICT_KEEP);
        r.h = std::min<uint32_t>(lens[d], 32768u);
        r.hs = compress_wave_digest_hs(r.h);
        r.end = set->mem + at_bytes[d] + r.kept;
        r.digest = set->mem + at_digest + dg * d;
        if (r.kept)
            e = hipMemcpyAsync(set->mem + at_bytes[d], (const uint8_t*)dict_base + offs[d] + (lens[d] - r.kept), r.kept,
                               mem_kind == LZ4FLEX_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s);
    }
    // (pageable host memory: hipMemcpyAsync has read the caller's bytes, and `table`, when it returns)
    if (e == hipSuccess) e = hipMemcpyAsync(set->mem + at_table, table.data(), sizeof(DictSetRec) * (size_t)k, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(set->mem + at_counter, 0, 4, s);
    set->table = (const DictSetRec*)(set->mem + at_table);
    set->counter = (uint32_t*)(set->mem + at_counter);
    if (e == hipSuccess) e = launch_dict_set_digests(set->table, k, scratch, s);
    const hipError_t w = hipStreamSynchronize(s);      // (also behind a failure: nothing of this call is in flight when its memory goes)
    if (e == hipSuccess) e = w;
    if (scratch) (void)hipFree(scratch);
    if (e != hipSuccess) {
        rc = hip_fail(e, "dict_set_create");
        if (set->mem) (void)hipFree(set->mem);
        delete set;
        return e == hipErrorOutOfMemory ? -LZ4FLEX_E_NOMEM : rc;
    }
    {
        std::lock_guard<std::mutex> lock(g_sets_mu);
        g_live_sets.push_back(set);
    }
    *out = set;
    return 0;
}

void lz4flex_dict_set_free(lz4flex_dict_set* set) {
    if (!set) return;
    {
        std::lock_guard<std::mutex> lock(g_sets_mu);
        g_live_sets.erase(std::remove(g_live_sets.begin(), g_live_sets.end(), set), g_live_sets.end());
    }
    if (set->mem) {
        DeviceGuard guard(set->device);
        (void)hipFree(set->mem);
    }
    delete set;
}

uint32_t lz4flex_dict_set_count(const lz4flex_dict_set* set) { return set ? set->k : 0u; }

// what the two *_dict_set entries share: the checks in their order, then the batch
static int run_dict_set_batch(lz4flex_ctx* ctx, BatchCall& b, const uint32_t* dict_id, const lz4flex_dict_set* set, int mem_kind, int host_flags) {
    if (!batch_arrays_ok(b) || (b.n && (!dict_id || !set))) return -LZ4FLEX_E_INVALID_ARG;
    const MemKind k = classify_mem(mem_kind, host_flags, LZ4FLEX_MEM_BIG_BLOCKS);     // (no LZ4FLEX_MEM_CHAINED)
    if (k.where == Mem::Invalid) return -LZ4FLEX_E_INVALID_ARG;
    // "debug_dict_set_items" speaks of THIS call from here on: one that has nothing to do or is refused below counts nothing
    if (b.compress)
        if (lz4flex_ctx* c0 = ctx ? ctx : g_default_ctx) c0->set_counted = nullptr;
    if (b.n == 0) return 0;
    b.has_ext = true; b.set = set; b.dict_id = dict_id;
    const int rc = begin_batch(&ctx);
    if (rc) return rc;
    if (ctx->device != set->device) { g_last_error = "the dictionary set belongs to another device"; return -LZ4FLEX_E_INVALID_ARG; }
    return run_batch(ctx, b, k);
}

int lz4flex_compress_batch_dict_set(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len, uint32_t n,
                                    const uint32_t* dict_id, void* out_base, const uint64_t* out_off, const uint32_t* out_cap,
                                    uint32_t* out_len, int32_t* status, const lz4flex_dict_set* set, int mem_kind, void* hip_stream) {
    BatchCall b = batch_of(true, in_base, in_off, in_len, n, out_base, out_off, out_cap, out_len, status, hip_stream);
    return run_dict_set_batch(ctx, b, dict_id, set, mem_kind, 0);
}

int lz4flex_decompress_batch_dict_set(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len, uint32_t n,
                                      const uint32_t* dict_id, void* out_base, const uint64_t* out_off, const uint32_t* out_cap,
                                      uint32_t* out_len, int32_t* status, uint64_t* detail, const lz4flex_dict_set* set, int mem_kind,
                                      void* hip_stream) {
    BatchCall b = batch_of(false, in_base, in_off, in_len, n, out_base, out_off, out_cap, out_len, status, hip_stream);
    b.detail = detail;
    return run_dict_set_batch(ctx, b, dict_id, set, mem_kind, LZ4FLEX_MEM_BIG_BLOCKS);
}

int lz4flex_decompress_batch_partial_dict_set(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len, uint32_t n,
                                              const uint32_t* dict_id, void* out_base, const uint64_t* out_off, const uint32_t* target,
                                              uint32_t* out_len, int32_t* status, const lz4flex_dict_set* set, int mem_kind, void* hip_stream) {
    BatchCall b = batch_of(false, in_base, in_off, in_len, n, out_base, out_off, target, out_len, status, hip_stream);
    b.partial = true;
    return run_dict_set_batch(ctx, b, dict_id, set, mem_kind, LZ4FLEX_MEM_BIG_BLOCKS);
}

int lz4flex_decompress_batch(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len,
                             uint32_t n, void* out_base, const uint64_t* out_off, const uint32_t* out_cap,
                             uint32_t* out_len, int32_t* status, uint64_t* detail, int mem_kind, void* hip_stream) {
    return lz4flex_decompress_batch_ex(ctx, in_base, in_off, in_len, n, out_base, out_off, out_cap, out_len, status,
                                       detail, nullptr, mem_kind, hip_stream);
}

// The sizes of raw blocks (lz4_size_scan.hip).  HOST: the input span and the descriptors go up in one staging layout, the results come
// back to page-locked memory, one synchronisation.  DEVICE: two launches on the caller's stream, nothing else.
int lz4flex_decompressed_size_batch(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len, uint32_t n,
                                    const uint32_t* history, uint64_t* out_size, int32_t* status, int mem_kind, void* hip_stream) {
    int rc;
    if ((rc = ctx_resolve(&ctx))) return rc;
    const MemKind k = classify_mem(mem_kind, LZ4FLEX_MEM_BIG_BLOCKS, LZ4FLEX_MEM_BIG_BLOCKS);
    if (k.where == Mem::Invalid) return -LZ4FLEX_E_INVALID_ARG;
    if (n == 0) return 0;
    if (!in_off || !in_len || !out_size || !status) return -LZ4FLEX_E_INVALID_ARG;
    if ((rc = injected_failure(ctx))) return rc;
    if (k.where == Mem::Device) {
        const hipError_t le = launch_size_scan((const uint8_t*)in_base, in_off, in_len, history, n, out_size, status, ctx->size_serial,
                                               (hipStream_t)hip_stream);
        return le != hipSuccess ? hip_fail(le, "size scan launch") : 0;
    }
    DeviceGuard guard(ctx->device);
    HIP_TRY(guard.err);
    const Span sp = span_of(in_off, in_len, n);
    HostStage st;
    const auto c_off = st.up<uint64_t>(n);
    const auto c_len = st.up<uint32_t>(n), c_hist = st.up<uint32_t>(history ? n : 0);
    const auto c_size = st.down<uint64_t>(n);
    const auto c_status = st.down<int32_t>(n);
    const Region r_in = st.region(sp.bytes(), 64);
    st.columns();
    if ((rc = stage_open(ctx, st))) return rc;
    st.fill_offsets(c_off, in_off, sp.lo); st.fill(c_len, in_len); st.fill(c_hist, history);
    HIP_TRY(st.send(r_in, (const uint8_t*)in_base + sp.lo));
    HIP_TRY(st.send_columns());
    const hipError_t le = launch_size_scan(st.dev(r_in), st.dev(c_off), st.dev(c_len), st.dev_opt(c_hist), n, st.dev(c_size), st.dev(c_status),
                                           ctx->size_serial, st.s);
    if (le != hipSuccess) return hip_fail(le, "size scan launch");
    HIP_TRY(st.fetch_columns(c_size));
    HIP_TRY(hipStreamSynchronize(st.s));
    st.read(c_size, out_size); st.read(c_status, status);
    return 0;
}

// ---- packed batches: ONE output buffer, the layout computed on the device (lz4_packed.hip) -----------------------------------
}  // extern "C"

namespace {

bool packed_align_ok(uint32_t a) { return a >= 1u && a <= 256u && (a & (a - 1u)) == 0u; }

// everything the public decode entry takes, as device pointers
struct PackedDecode {
    const uint8_t* in_base; const uint64_t* in_off; const uint32_t* in_len; uint32_t n; int size_mode; const uint32_t* sizes;
    uint8_t* out_base; uint64_t total_cap; uint32_t align; uint64_t* out_off; uint32_t* out_cap; uint32_t* out_len; int32_t* status;
    uint64_t* detail; void* work; bool big; hipStream_t stream;
};
// the slot sizes, out_off[0 .. n], out_cap and the blocks without size or room (PackedWork::pre): three small launches (SCAN: behind
// the size pass)
int packed_decode_layout(lz4flex_ctx* c, const PackedDecode& d) {
    const PackedWork w = packed_work(d.work, d.n);
    hipError_t e = hipSuccess;
    if (d.size_mode == LZ4FLEX_SIZES_SCAN) e = launch_size_scan(d.in_base, d.in_off, d.in_len, nullptr, d.n, w.size, w.pre, c->size_serial, d.stream);
    if (e == hipSuccess) e = launch_packed_sizes(d.size_mode, d.in_base, d.in_off, d.in_len, d.sizes, nullptr, d.n, 0u, w.size, w.aux_off, w.aux_len, w.pre, d.stream);
    if (e == hipSuccess) e = launch_packed_scan(w.size, d.n, d.align, d.total_cap, 0u, w.tiles, d.out_off, w.place, d.out_cap, w.pre, d.stream);
    return e != hipSuccess ? hip_fail(e, "packed layout launch") : 0;
}
// the decoder on the slots (a block without size or room has capacity 0: nothing of it is written), then those blocks' own status
int packed_decode_run(lz4flex_ctx* c, const PackedDecode& d) {
    const PackedWork w = packed_work(d.work, d.n);
    const bool prepended = d.size_mode == LZ4FLEX_SIZES_PREPENDED;
    BatchCall b = batch_of(false, d.in_base, prepended ? w.aux_off : d.in_off, prepended ? w.aux_len : d.in_len, d.n, d.out_base, w.place,
                           d.out_cap, d.out_len, d.status, d.stream);
    b.detail = d.detail; b.big = d.big;
    const int rc = run_device_batch(c, b);
    if (rc) return rc;
    const hipError_t e = launch_packed_finish(w.pre, w.size, d.out_off, d.n, d.total_cap, d.out_len, d.status, d.detail, d.stream);
    return e != hipSuccess ? hip_fail(e, "packed finish launch") : 0;
}

struct PackedCompress {
    const uint8_t* in_base; const uint64_t* in_off; const uint32_t* in_len; uint32_t n; uint32_t prefix; uint8_t* scratch; uint64_t scratch_cap;
    uint8_t* out_base; uint64_t total_cap; uint32_t align; uint64_t* out_off; uint32_t* out_len; int32_t* status; void* work; bool big;
    hipStream_t stream;
};
// scratch slots of get_maximum_output_size (+ prefix) bytes back to back, the encoder into them, the produced lengths scanned into
// out_off, the gather.  A slot beyond scratch_cap has capacity 0: the encoder answers OUTPUT_TOO_SMALL for that block.
int packed_compress_run(lz4flex_ctx* c, const PackedCompress& d) {
    const PackedWork w = packed_work(d.work, d.n);
    hipStream_t s = d.stream;
    hipError_t e = launch_packed_sizes(PACKED_SIZES_SLOTS, d.in_base, d.in_off, d.in_len, nullptr, nullptr, d.n, d.prefix, w.size, nullptr, nullptr, w.pre, s);
    if (e == hipSuccess) e = launch_packed_scan(w.size, d.n, 1u, d.scratch_cap, d.prefix, w.tiles, w.aux_off, w.place, w.aux_len, w.pre, s);
    if (e == hipSuccess) e = hipMemsetAsync(d.out_len, 0, 4ull * d.n, s);
    if (e == hipSuccess) e = hipMemsetAsync(d.status, 0, 4ull * d.n, s);
    if (e != hipSuccess) return hip_fail(e, "packed layout launch");
    BatchCall b = batch_of(true, d.in_base, d.in_off, d.in_len, d.n, d.scratch, w.place, w.aux_len, d.out_len, d.status, s);
    b.big = d.big;
    const int rc = run_device_batch(c, b);
    if (rc) return rc;
    e = launch_packed_sizes(PACKED_SIZES_PRODUCED, nullptr, nullptr, nullptr, d.out_len, d.status, d.n, d.prefix, w.size, nullptr, nullptr, nullptr, s);
    if (e == hipSuccess) e = launch_packed_scan(w.size, d.n, d.align, d.total_cap, 0u, w.tiles, d.out_off, nullptr, nullptr, nullptr, s);
    if (e == hipSuccess) e = launch_packed_gather(d.scratch, w.place, w.size, d.out_off, d.in_len, d.n, d.prefix, d.total_cap, d.out_base, d.out_len, d.status, s);
    return e != hipSuccess ? hip_fail(e, "packed gather launch") : 0;
}

// MEM_HOST: the produced bytes [0, used) of the device buffer come down in one transfer; every good block's bytes go to their place in
// the caller's buffer (the gaps between blocks and everything behind them stay the caller's)
int packed_scatter_to_host(lz4flex_ctx* c, const uint8_t* d_out, uint64_t used, uint8_t* out_base, const uint64_t* off, const uint32_t* len,
                           const int32_t* st, uint32_t n) {
    if (!used) return 0;
    int rc;
    if ((rc = ensure_buf(c->pay, (size_t)used))) return rc;
    HIP_TRY(hipMemcpyAsync(c->pay.p, d_out, (size_t)used, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    scatter_good(out_base, off, len, st, n, c->pay.p, [&](uint32_t i) { return off[i]; }, used);
    return 0;
}

}  // namespace

extern "C" {

size_t lz4flex_packed_work_size(uint32_t n) { return packed_work_bytes(n); }

uint64_t lz4flex_compress_packed_scratch_bound(uint64_t total_in_bytes, uint32_t n, int prepend_size) {
    // sum of floor(len_i * 110 / 100) <= floor(total * 110 / 100)
    return total_in_bytes / 100u * 110u + (total_in_bytes % 100u) * 110u / 100u + (uint64_t)n * (20u + (prepend_size ? 4u : 0u));
}

int lz4flex_decompress_batch_packed(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len, uint32_t n,
                                    int size_mode, const uint32_t* sizes, void* out_base, uint64_t total_cap, uint32_t align,
                                    uint64_t* out_off, uint32_t* out_cap, uint32_t* out_len, int32_t* status, uint64_t* detail, void* work,
                                    int mem_kind, void* hip_stream) {
    if (size_mode != LZ4FLEX_SIZES_PREPENDED && size_mode != LZ4FLEX_SIZES_GIVEN && size_mode != LZ4FLEX_SIZES_SCAN) return -LZ4FLEX_E_INVALID_ARG;
    if (!packed_align_ok(align)) return -LZ4FLEX_E_INVALID_ARG;
    const MemKind k = classify_mem(mem_kind, LZ4FLEX_MEM_BIG_BLOCKS, LZ4FLEX_MEM_BIG_BLOCKS);     // (no LZ4FLEX_MEM_CHAINED)
    if (k.where == Mem::Invalid) return -LZ4FLEX_E_INVALID_ARG;
    if (n == 0) return 0;
    if (!in_off || !in_len || !out_off || !out_cap || !out_len || !status) return -LZ4FLEX_E_INVALID_ARG;
    if (size_mode == LZ4FLEX_SIZES_GIVEN && !sizes) return -LZ4FLEX_E_INVALID_ARG;
    if (k.where == Mem::Device && !work) return -LZ4FLEX_E_INVALID_ARG;
    int rc;
    if ((rc = begin_batch(&ctx))) return rc;
    PackedDecode d{(const uint8_t*)in_base, in_off, in_len, n, size_mode, sizes, (uint8_t*)out_base, total_cap, align, out_off, out_cap,
                   out_len, status, detail, work, k.big, (hipStream_t)hip_stream};
    if (k.where == Mem::Device) return (rc = packed_decode_layout(ctx, d)) ? rc : packed_decode_run(ctx, d);

    // MEM_HOST: the work area behind the columns; the output buffer (scratch slot 0) is sized once the layout is known
    lz4flex_ctx* c = ctx;
    DeviceGuard guard(c->device);
    HIP_TRY(guard.err);
    const Span sp = span_of(in_off, in_len, n);
    HostStage st;
    const auto c_in_off = st.up<uint64_t>(n);
    const auto c_in_len = st.up<uint32_t>(n), c_sizes = st.up<uint32_t>(size_mode == LZ4FLEX_SIZES_GIVEN ? n : 0);
    const auto c_out_off = st.down<uint64_t>(n + 1ull);
    const auto c_out_cap = st.down<uint32_t>(n), c_out_len = st.down<uint32_t>(n);
    const auto c_status = st.down<int32_t>(n);
    const auto c_detail = st.down<uint64_t>(2ull * n);
    const Region r_in = st.region(sp.bytes(), 64);
    st.columns();
    const Region r_work = st.region(packed_work_bytes(n), 0);
    if ((rc = stage_open(c, st))) return rc;
    st.fill_offsets(c_in_off, in_off, sp.lo); st.fill(c_in_len, in_len); st.fill(c_sizes, sizes);
    hipStream_t s = st.s;
    HIP_TRY(st.send(r_in, (const uint8_t*)in_base + sp.lo));
    HIP_TRY(st.send_columns());
    d.in_base = st.dev(r_in); d.in_off = st.dev(c_in_off); d.in_len = st.dev(c_in_len); d.sizes = st.dev_opt(c_sizes);
    d.out_off = st.dev(c_out_off); d.out_cap = st.dev(c_out_cap); d.out_len = st.dev(c_out_len);
    d.status = st.dev(c_status); d.detail = st.dev(c_detail); d.work = st.dev(r_work); d.stream = s;
    d.big = k.big || host_big(in_len, n, false);
    if ((rc = packed_decode_layout(c, d))) return rc;
    uint64_t need = 0;
    HIP_TRY(hipMemcpyAsync(&need, d.out_off + n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t used = std::min<uint64_t>(need, total_cap);
    void* d_out = nullptr;
    if ((rc = ctx_scratch(c, 0, (size_t)used + 256, &d_out))) return rc;
    d.out_base = (uint8_t*)d_out;
    if ((rc = packed_decode_run(c, d))) return rc;
    HIP_TRY(st.fetch_columns(c_out_off));
    HIP_TRY(hipStreamSynchronize(s));
    st.read(c_out_off, out_off); st.read(c_out_cap, out_cap); st.read(c_out_len, out_len); st.read(c_status, status);
    if (detail) st.read(c_detail, detail);
    return packed_scatter_to_host(c, (const uint8_t*)d_out, used, (uint8_t*)out_base, out_off, out_len, status, n);
}

int lz4flex_compress_batch_packed(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len, uint32_t n,
                                  int prepend_size, void* scratch, uint64_t scratch_cap, void* out_base, uint64_t total_cap, uint32_t align,
                                  uint64_t* out_off, uint32_t* out_len, int32_t* status, void* work, int mem_kind, void* hip_stream) {
    if (!packed_align_ok(align)) return -LZ4FLEX_E_INVALID_ARG;
    const MemKind k = classify_mem(mem_kind, LZ4FLEX_MEM_BIG_BLOCKS, LZ4FLEX_MEM_BIG_BLOCKS);
    if (k.where == Mem::Invalid) return -LZ4FLEX_E_INVALID_ARG;
    if (n == 0) return 0;
    if (!in_off || !in_len || !out_off || !out_len || !status) return -LZ4FLEX_E_INVALID_ARG;
    if (k.where == Mem::Device && (!work || !scratch)) return -LZ4FLEX_E_INVALID_ARG;
    const uint32_t prefix = prepend_size ? 4u : 0u;
    uint64_t slots = 0, packed_bound = 0;
    bool big = k.big;
    if (k.where == Mem::Host) {                       // the lengths are visible: the scratch a DEVICE call of this batch would need
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t slot = lz4flex_get_maximum_output_size(in_len[i]) + prefix;
            slots += slot;
            packed_bound += (slot + align - 1u) & ~(uint64_t)(align - 1u);
        }
        big = big || host_big(in_len, n, true);
        if (scratch_cap < slots) return -LZ4FLEX_E_INVALID_ARG;
    }
    int rc;
    if ((rc = begin_batch(&ctx))) return rc;
    PackedCompress d{(const uint8_t*)in_base, in_off, in_len, n, prefix, (uint8_t*)scratch, scratch_cap, (uint8_t*)out_base, total_cap, align,
                     out_off, out_len, status, work, big, (hipStream_t)hip_stream};
    if (k.where == Mem::Device) return packed_compress_run(ctx, d);

    // MEM_HOST: the work area behind the columns, the scratch slots and the packed stream in the context's scratch slots 0 and 1
    lz4flex_ctx* c = ctx;
    DeviceGuard guard(c->device);
    HIP_TRY(guard.err);
    const Span sp = span_of(in_off, in_len, n);
    HostStage st;
    const auto c_in_off = st.up<uint64_t>(n);
    const auto c_in_len = st.up<uint32_t>(n);
    const auto c_out_off = st.down<uint64_t>(n + 1ull);
    const auto c_out_len = st.down<uint32_t>(n);
    const auto c_status = st.down<int32_t>(n);
    const Region r_in = st.region(sp.bytes(), 64);
    st.columns();
    const Region r_work = st.region(packed_work_bytes(n), 0);
    if ((rc = stage_open(c, st))) return rc;
    const uint64_t out_bytes = std::min<uint64_t>(packed_bound, total_cap);
    void *d_scratch = nullptr, *d_out = nullptr;
    if ((rc = ctx_scratch(c, 0, (size_t)slots + 256, &d_scratch))) return rc;
    if ((rc = ctx_scratch(c, 1, (size_t)out_bytes + 256, &d_out))) return rc;
    st.fill_offsets(c_in_off, in_off, sp.lo); st.fill(c_in_len, in_len);
    HIP_TRY(st.send(r_in, (const uint8_t*)in_base + sp.lo));
    HIP_TRY(st.send_columns());
    d.in_base = st.dev(r_in); d.in_off = st.dev(c_in_off); d.in_len = st.dev(c_in_len);
    d.scratch = (uint8_t*)d_scratch; d.scratch_cap = slots; d.out_base = (uint8_t*)d_out;
    d.out_off = st.dev(c_out_off); d.out_len = st.dev(c_out_len); d.status = st.dev(c_status);
    d.work = st.dev(r_work); d.stream = st.s;
    if ((rc = packed_compress_run(c, d))) return rc;
    HIP_TRY(st.fetch_columns(c_out_off));
    HIP_TRY(hipStreamSynchronize(st.s));
    st.read(c_out_off, out_off); st.read(c_out_len, out_len); st.read(c_status, status);
    return packed_scatter_to_host(c, (const uint8_t*)d_out, std::min<uint64_t>(out_off[n], out_bytes), (uint8_t*)out_base, out_off, out_len, status, n);
}

// ---- a dictionary from a batch of samples (lz4_dict_train.hip) -------------------------------------------------------------------
size_t lz4flex_dict_train_work_size(uint32_t n) { return dict_train_work_bytes(n); }

// DEVICE: the launches on the caller's stream, nothing else.  HOST: one transfer down (the two words and dict_cap bytes), one synchronisation.
int lz4flex_dict_train(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len, uint32_t n, void* dict_out,
                       uint32_t dict_cap, uint32_t segment, uint32_t* dict_len, int32_t* status, void* work, int mem_kind, void* hip_stream) {
    if (segment != 0u && (segment < 64u || segment > 2048u)) return -LZ4FLEX_E_INVALID_ARG;
    if (dict_cap > DICT_KEEP || !dict_len || !status || (dict_cap && !dict_out)) return -LZ4FLEX_E_INVALID_ARG;
    if (n && (!in_off || !in_len)) return -LZ4FLEX_E_INVALID_ARG;
    const MemKind k = classify_mem(mem_kind, LZ4FLEX_MEM_BIG_BLOCKS, LZ4FLEX_MEM_BIG_BLOCKS);     // (no LZ4FLEX_MEM_CHAINED; BIG_BLOCKS changes nothing)
    if (k.where == Mem::Invalid) return -LZ4FLEX_E_INVALID_ARG;
    if (k.where == Mem::Device && !work) return -LZ4FLEX_E_INVALID_ARG;
    const uint32_t seg = segment ? segment : 512u;
    const bool nothing = n == 0u || dict_cap == 0u;
    if (nothing && k.where == Mem::Host) { *dict_len = 0u; *status = 0; return 0; }
    int rc;
    if ((rc = begin_batch(&ctx))) return rc;
    if (k.where == Mem::Device) {
        const hipError_t le = launch_dict_train((const uint8_t*)in_base, in_off, in_len, n, (uint8_t*)dict_out, dict_cap, seg, dict_len, status,
                                                work, (hipStream_t)hip_stream);
        return le != hipSuccess ? hip_fail(le, "dict train launch") : 0;
    }
    DeviceGuard guard(ctx->device);
    HIP_TRY(guard.err);
    const Span sp = span_of(in_off, in_len, n);
    HostStage st;
    const auto c_in_off = st.up<uint64_t>(n);
    const auto c_in_len = st.up<uint32_t>(n);
    const auto c_res = st.down<uint32_t>(2);                  // two words side by side: the length, the status
    const auto c_dict = st.down<uint8_t>(dict_cap);
    const Region r_in = st.region(sp.bytes(), 64);
    st.columns();
    const Region r_work = st.region(dict_train_work_bytes(n), 0);
    if ((rc = stage_open(ctx, st))) return rc;
    st.fill_offsets(c_in_off, in_off, sp.lo); st.fill(c_in_len, in_len);
    HIP_TRY(st.send(r_in, (const uint8_t*)in_base + sp.lo));
    HIP_TRY(st.send_columns());
    const hipError_t le = launch_dict_train(st.dev(r_in), st.dev(c_in_off), st.dev(c_in_len), n, st.dev(c_dict), dict_cap, seg, st.dev(c_res),
                                            (int32_t*)(st.dev(c_res) + 1), st.dev(r_work), st.s);
    if (le != hipSuccess) return hip_fail(le, "dict train launch");
    HIP_TRY(st.fetch_columns(c_res));
    HIP_TRY(hipStreamSynchronize(st.s));
    *dict_len = st.host(c_res)[0];
    *status = (int32_t)st.host(c_res)[1];
    if (*dict_len) st.read(c_dict, (uint8_t*)dict_out, std::min<uint32_t>(*dict_len, dict_cap));
    return 0;
}

// ---- typed batches: the shuffle / bitshuffle filters around the codec (lz4_filter.hip) ------------------------------------------------
}  // extern "C"

namespace {

enum class Typed { Filter, Compress, Decompress };

static_assert(LZ4FLEX_FILTER_DELTA == FILTER_DELTA && LZ4FLEX_DELTA_RESTART == FILTER_TILE_ELEMS, "the header's delta constants are the kernels'");

bool filter_args_ok(int filter, uint32_t elem) {
    if (filter < 0 || (filter & ~(LZ4FLEX_FILTER_DELTA | 3)) != 0) return false;
    const int base = filter & ~LZ4FLEX_FILTER_DELTA;     // the flag rides on the value: launch_filter takes them together
    return (base == LZ4FLEX_FILTER_NONE || base == LZ4FLEX_FILTER_SHUFFLE || base == LZ4FLEX_FILTER_BITSHUFFLE) &&
           (elem == 1u || elem == 2u || elem == 4u || elem == 8u);
}

int launch_filter_checked(lz4flex_ctx* c, const uint8_t* in_base, const uint64_t* in_off, const uint32_t* len, const int32_t* gate, uint8_t* out_base,
                          const uint64_t* out_off, uint32_t n, int filter, uint32_t elem, bool inverse, hipStream_t s) {
    const FilterArgs f{in_base, in_off, len, gate, out_base, out_off, n, (uint32_t)c->filter_bytewise};
    const hipError_t le = launch_filter(f, filter, elem, inverse, s);
    return le != hipSuccess ? hip_fail(le, "filter launch") : 0;
}

// One typed call on device memory, b holding the call's arrays (Filter: no out_cap / out_len / status).  Compress: the forward filter
// into the tmp slots, the encoders on the slots.  Decompress: the decoders into the tmp slots, the inverse filter over out_len[i] bytes of
// every block with status 0, read from the device arrays on the same stream.
int typed_on_device(lz4flex_ctx* c, Typed op, BatchCall b, int filter, uint32_t elem, bool inverse, uint8_t* tmp_base, const uint64_t* tmp_off) {
    hipStream_t s = b.stream;
    if (op == Typed::Filter) return launch_filter_checked(c, b.in_base, b.in_off, b.in_len, nullptr, b.out_base, b.out_off, b.n, filter, elem, inverse, s);
    if (op == Typed::Compress) {
        if (const int rc = launch_filter_checked(c, b.in_base, b.in_off, b.in_len, nullptr, tmp_base, tmp_off, b.n, filter, elem, false, s)) return rc;
        return compress_batch_entry(c, tmp_base, tmp_off, b.in_len, nullptr, b.n, b.out_base, b.out_off, b.out_cap, b.out_len, b.status,
                                    LZ4FLEX_MEM_DEVICE | (b.big ? LZ4FLEX_MEM_BIG_BLOCKS : 0), s, false);
    }
    uint8_t* const out_base = b.out_base;
    const uint64_t* const out_off = b.out_off;
    b.out_base = tmp_base; b.out_off = tmp_off;
    if (const int rc = run_device_batch(c, b)) return rc;
    return launch_filter_checked(c, tmp_base, tmp_off, b.out_len, b.status, out_base, out_off, b.n, filter, elem, true, s);
}

// MEM_HOST: the tmp slots mirror the input span (compress) or the output span (decompress); one synchronisation; the output span comes
// down to page-locked memory and every block that has bytes (Filter: all of them; else status 0) is copied to its place, the rest of the
// caller's buffer stays as it is.
int typed_on_host(lz4flex_ctx* c, Typed op, const BatchCall& b, int filter, uint32_t elem, bool inverse, bool big) {
    const uint32_t n = b.n;
    DeviceGuard guard(c->device);
    HIP_TRY(guard.err);
    const bool codec = op != Typed::Filter;
    const Span in_span = span_of(b.in_off, b.in_len, n);
    const Span out_span = span_of(b.out_off, codec ? b.out_cap : b.in_len, n);
    const size_t in_bytes = in_span.bytes(), out_bytes = out_span.bytes();
    HostStage st;
    const auto in_off = st.up<uint64_t>(n), out_off = st.up<uint64_t>(n), tmp_off = st.up<uint64_t>(n);
    const auto in_len = st.up<uint32_t>(n), out_cap = st.up<uint32_t>(n);
    const auto out_len = st.down<uint32_t>(n);
    const auto status = st.down<int32_t>(n);
    const auto detail = st.down<uint64_t>(2ull * n);
    const Region r_in = st.region(in_bytes, 64), r_tmp = st.region(op == Typed::Compress ? in_bytes : op == Typed::Decompress ? out_bytes : 0, 64),
                 r_out = st.region(out_bytes, 64);
    st.columns();
    int rc;
    if ((rc = stage_open(c, st))) return rc;
    if ((rc = ensure_buf(c->pay, out_bytes + 16))) return rc;
    st.fill_offsets(in_off, b.in_off, in_span.lo); st.fill_offsets(out_off, b.out_off, out_span.lo);
    if (op == Typed::Compress) st.fill_offsets(tmp_off, b.in_off, in_span.lo); else st.fill_offsets(tmp_off, b.out_off, out_span.lo);
    st.fill(in_len, b.in_len);
    if (codec) st.fill(out_cap, b.out_cap); else st.zero(out_cap);
    hipStream_t s = st.s;
    HIP_TRY(st.send(r_in, b.in_base + in_span.lo));
    HIP_TRY(st.send_columns());
    BatchCall dv = batch_of(op == Typed::Compress, st.dev(r_in), st.dev(in_off), st.dev(in_len), n, st.dev(r_out), st.dev(out_off), st.dev(out_cap),
                            st.dev(out_len), st.dev(status), s);
    dv.big = big;
    if (op == Typed::Decompress) dv.detail = st.dev(detail);
    if ((rc = typed_on_device(c, op, dv, filter, elem, inverse, st.dev(r_tmp), st.dev(tmp_off)))) return rc;
    if (codec) HIP_TRY(st.fetch_columns(out_len));
    if (out_bytes) HIP_TRY(hipMemcpyAsync(c->pay.p, st.dev(r_out), out_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (codec) copy_results(b, st.host(out_len), st.host(status), st.host(detail));
    scatter_good(b.out_base, b.out_off, codec ? st.host(out_len) : b.in_len, codec ? st.host(status) : nullptr, n, c->pay.p,
                 [&](uint32_t i) { return b.out_off[i] - out_span.lo; });
    return 0;
}

// what the three typed entries share: their checks in their order (arguments, then the context), then the memory kind's path
int typed_entry(lz4flex_ctx* ctx, Typed op, BatchCall b, int filter, uint32_t elem, bool inverse, void* tmp_base, const uint64_t* tmp_off, int mem_kind) {
    if (!filter_args_ok(filter, elem)) return -LZ4FLEX_E_INVALID_ARG;
    const MemKind k = classify_mem(mem_kind, LZ4FLEX_MEM_BIG_BLOCKS, LZ4FLEX_MEM_BIG_BLOCKS);     // (no LZ4FLEX_MEM_CHAINED; Filter: BIG_BLOCKS changes nothing)
    if (k.where == Mem::Invalid) return -LZ4FLEX_E_INVALID_ARG;
    if (b.n == 0) return 0;
    if (!b.in_off || !b.in_len || !b.out_off) return -LZ4FLEX_E_INVALID_ARG;
    if (op != Typed::Filter && (!b.out_cap || !b.out_len || !b.status)) return -LZ4FLEX_E_INVALID_ARG;
    const bool slots = op != Typed::Filter && filter != LZ4FLEX_FILTER_NONE;
    if (slots && k.where == Mem::Device && (!tmp_base || !tmp_off)) return -LZ4FLEX_E_INVALID_ARG;
    int rc;
    if ((rc = ctx_resolve(&ctx))) return rc;
    if (!(op == Typed::Compress && slots) && (rc = injected_failure(ctx))) return rc;     // (compress_batch_entry has the hook of a filtered compress)
    if (op != Typed::Filter && !slots) {               // FILTER_NONE: the plain entry's path, tmp is not touched
        b.big = k.big;
        return k.where == Mem::Host ? run_host_batch(ctx, b) : run_device_batch(ctx, b);
    }
    if (k.where == Mem::Device) { b.big = k.big; return typed_on_device(ctx, op, b, filter, elem, inverse, (uint8_t*)tmp_base, tmp_off); }
    return typed_on_host(ctx, op, b, filter, elem, inverse, k.big || (op != Typed::Filter && host_big(b.in_len, b.n, b.compress)));
}

}  // namespace

extern "C" {

int lz4flex_filter_batch(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len, uint32_t n, void* out_base,
                         const uint64_t* out_off, int filter, uint32_t elem_size, int inverse, int mem_kind, void* hip_stream) {
    const BatchCall b = batch_of(false, in_base, in_off, in_len, n, out_base, out_off, nullptr, nullptr, nullptr, hip_stream);
    return typed_entry(ctx, Typed::Filter, b, filter, elem_size, inverse != 0, nullptr, nullptr, mem_kind);
}

int lz4flex_compress_batch_typed(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len, uint32_t n, void* out_base,
                                 const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len, int32_t* status, int filter,
                                 uint32_t elem_size, void* tmp_base, const uint64_t* tmp_off, int mem_kind, void* hip_stream) {
    const BatchCall b = batch_of(true, in_base, in_off, in_len, n, out_base, out_off, out_cap, out_len, status, hip_stream);
    return typed_entry(ctx, Typed::Compress, b, filter, elem_size, false, tmp_base, tmp_off, mem_kind);
}

int lz4flex_decompress_batch_typed(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len, uint32_t n, void* out_base,
                                   const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len, int32_t* status, uint64_t* detail, int filter,
                                   uint32_t elem_size, void* tmp_base, const uint64_t* tmp_off, int mem_kind, void* hip_stream) {
    BatchCall b = batch_of(false, in_base, in_off, in_len, n, out_base, out_off, out_cap, out_len, status, hip_stream);
    b.detail = detail;
    return typed_entry(ctx, Typed::Decompress, b, filter, elem_size, true, tmp_base, tmp_off, mem_kind);
}

// ---- fit batches: a finished block cut to a capacity (lz4_fit.hip) -------------------------------------------------------------------
}  // extern "C"

namespace {

int launch_fit_checked(lz4flex_ctx* c, const FitArgs& a, bool gated, hipStream_t s) {
    const hipError_t le = launch_fit(a, gated ? 1 : 0, c->fit_first_pass ? 2 : c->fit_serial, s);
    return le != hipSuccess ? hip_fail(le, "fit launch") : 0;
}

// lz4flex_compress_batch_fit on device memory (a.blk_* are this function's to fill): scratch slots of get_maximum_output_size bytes back to
// back, their offsets scanned on the device (lz4_packed.hip), the encoder into them, the fit pass from them.  A slot beyond scratch_cap
// has capacity 0: the encoder answers OUTPUT_TOO_SMALL for that block and the fit pass leaves it at that.
int compress_fit_on_device(lz4flex_ctx* c, FitArgs a, uint8_t* scratch, uint64_t scratch_cap, void* work, bool big, hipStream_t s) {
    const PackedWork w = packed_work(work, a.n);
    uint32_t* const enc_len = (uint32_t*)w.size;             // (the sizes are read by the scan alone: the encoder's lengths take their place)
    hipError_t e = launch_packed_sizes(PACKED_SIZES_SLOTS, a.src_base, a.src_off, a.src_len, nullptr, nullptr, a.n, 0u, w.size, nullptr, nullptr, w.pre, s);
    if (e == hipSuccess) e = launch_packed_scan(w.size, a.n, 1u, scratch_cap, 0u, w.tiles, w.aux_off, w.place, w.aux_len, w.pre, s);
    if (e == hipSuccess) e = hipMemsetAsync(enc_len, 0, 4ull * a.n, s);
    if (e == hipSuccess) e = hipMemsetAsync(a.status, 0, 4ull * a.n, s);
    if (e != hipSuccess) return hip_fail(e, "fit layout launch");
    if (const int rc = compress_batch_entry(c, a.src_base, a.src_off, a.src_len, nullptr, a.n, scratch, w.place, w.aux_len, enc_len, a.status,
                                            LZ4FLEX_MEM_DEVICE | (big ? LZ4FLEX_MEM_BIG_BLOCKS : 0), s, false)) return rc;
    a.blk_base = scratch; a.blk_off = w.place; a.blk_len = enc_len;
    return launch_fit_checked(c, a, true, s);
}

// MEM_HOST, both entries (compress: no block span, a work area, the scratch slots in the context's scratch slot 0); one synchronisation;
// the output span comes down to page-locked memory and every block with status 0 is copied to its place, the rest of the caller's
// buffer stays as it is.
int fit_on_host(lz4flex_ctx* c, const FitArgs& a, bool compress, bool big) {
    const uint32_t n = a.n;
    DeviceGuard guard(c->device);
    HIP_TRY(guard.err);
    const Span blk_span = compress ? Span{0, 0} : span_of(a.blk_off, a.blk_len, n);
    const Span src_span = span_of(a.src_off, a.src_len, n);
    const Span out_span = span_of(a.out_off, a.out_cap, n);
    const size_t out_bytes = out_span.bytes();
    uint64_t slots = 0;
    if (compress) {
        for (uint32_t i = 0; i < n; i++) slots += lz4flex_get_maximum_output_size(a.src_len[i]);
        big = big || host_big(a.src_len, n, true);
    }
    HostStage st;
    const auto blk_off = st.up<uint64_t>(n), src_off = st.up<uint64_t>(n), out_off = st.up<uint64_t>(n);
    const auto blk_len = st.up<uint32_t>(n), src_len = st.up<uint32_t>(n), out_cap = st.up<uint32_t>(n);
    const auto out_len = st.down<uint32_t>(n), used = st.down<uint32_t>(n);
    const auto status = st.down<int32_t>(n);
    const Region r_blk = st.region(blk_span.bytes(), 64), r_src = st.region(src_span.bytes(), 64), r_out = st.region(out_bytes, 64);
    st.columns();
    const Region r_work = st.region(compress ? packed_work_bytes(n) : 0, 0);
    int rc;
    if ((rc = stage_open(c, st))) return rc;
    if ((rc = ensure_buf(c->pay, out_bytes + 16))) return rc;
    void* d_scratch = nullptr;
    if (compress && (rc = ctx_scratch(c, 0, (size_t)slots + 256, &d_scratch))) return rc;
    if (compress) { st.zero(blk_off); st.zero(blk_len); }
    else { st.fill_offsets(blk_off, a.blk_off, blk_span.lo); st.fill(blk_len, a.blk_len); }
    st.fill_offsets(src_off, a.src_off, src_span.lo); st.fill_offsets(out_off, a.out_off, out_span.lo);
    st.fill(src_len, a.src_len); st.fill(out_cap, a.out_cap);
    hipStream_t s = st.s;
    HIP_TRY(st.send(r_blk, a.blk_base + blk_span.lo));
    HIP_TRY(st.send(r_src, a.src_base + src_span.lo));
    HIP_TRY(st.send_columns());
    const FitArgs dv{st.dev(r_blk), st.dev(blk_off), st.dev(blk_len), st.dev(r_src), st.dev(src_off), st.dev(src_len), n, st.dev(r_out),
                     st.dev(out_off), st.dev(out_cap), st.dev(out_len), st.dev(used), st.dev(status)};
    if ((rc = compress ? compress_fit_on_device(c, dv, (uint8_t*)d_scratch, slots, st.dev(r_work), big, s) : launch_fit_checked(c, dv, false, s))) return rc;
    HIP_TRY(st.fetch_columns(out_len));
    if (out_bytes) HIP_TRY(hipMemcpyAsync(c->pay.p, st.dev(r_out), out_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    st.read(out_len, a.out_len); st.read(used, a.in_used); st.read(status, a.status);
    scatter_good(a.out_base, a.out_off, a.out_len, a.status, n, c->pay.p, [&](uint32_t i) { return a.out_off[i] - out_span.lo; });
    return 0;
}

}  // namespace

extern "C" {

int lz4flex_fit_batch(lz4flex_ctx* ctx, const void* blk_base, const uint64_t* blk_off, const uint32_t* blk_len, const void* src_base,
                      const uint64_t* src_off, const uint32_t* src_len, uint32_t n, void* out_base, const uint64_t* out_off, const uint32_t* out_cap,
                      uint32_t* out_len, uint32_t* in_used, int32_t* status, int mem_kind, void* hip_stream) {
    const MemKind k = classify_mem(mem_kind, LZ4FLEX_MEM_BIG_BLOCKS, LZ4FLEX_MEM_BIG_BLOCKS);     // (no LZ4FLEX_MEM_CHAINED; BIG_BLOCKS changes nothing)
    if (k.where == Mem::Invalid) return -LZ4FLEX_E_INVALID_ARG;
    if (n == 0) return 0;
    if (!blk_off || !blk_len || !src_off || !src_len || !out_off || !out_cap || !out_len || !in_used || !status) return -LZ4FLEX_E_INVALID_ARG;
    int rc;
    if ((rc = begin_batch(&ctx))) return rc;
    const FitArgs a{(const uint8_t*)blk_base, blk_off, blk_len, (const uint8_t*)src_base, src_off, src_len, n, (uint8_t*)out_base, out_off, out_cap,
                    out_len, in_used, status};
    return k.where == Mem::Device ? launch_fit_checked(ctx, a, false, (hipStream_t)hip_stream) : fit_on_host(ctx, a, false, false);
}

size_t lz4flex_compress_fit_work_size(uint32_t n) { return packed_work_bytes(n); }

int lz4flex_compress_batch_fit(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len, uint32_t n, void* scratch,
                               uint64_t scratch_cap, void* out_base, const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len,
                               uint32_t* in_used, int32_t* status, void* work, int mem_kind, void* hip_stream) {
    const MemKind k = classify_mem(mem_kind, LZ4FLEX_MEM_BIG_BLOCKS, LZ4FLEX_MEM_BIG_BLOCKS);     // (no LZ4FLEX_MEM_CHAINED)
    if (k.where == Mem::Invalid) return -LZ4FLEX_E_INVALID_ARG;
    if (n == 0) return 0;
    if (!in_off || !in_len || !out_off || !out_cap || !out_len || !in_used || !status) return -LZ4FLEX_E_INVALID_ARG;
    if (k.where == Mem::Device && (!work || !scratch)) return -LZ4FLEX_E_INVALID_ARG;
    int rc;
    if ((rc = ctx_resolve(&ctx))) return rc;                  // (compress_batch_entry has the "debug_fail_next_batch" hook)
    const FitArgs a{nullptr, nullptr, nullptr, (const uint8_t*)in_base, in_off, in_len, n, (uint8_t*)out_base, out_off, out_cap, out_len, in_used, status};
    if (k.where == Mem::Device) return compress_fit_on_device(ctx, a, (uint8_t*)scratch, scratch_cap, work, k.big, (hipStream_t)hip_stream);
    return fit_on_host(ctx, a, true, k.big);
}

// ---- paged streams: every stream cut into pages of page_size bytes, the loop on the device (lz4_paged.hip) ------------------------------
}  // extern "C"

namespace {

// Lfit(r, infinity) of the fit rule: the largest L with tail(L) <= r (r >= 1)
uint32_t lfit_unbounded(uint32_t r) { return lz4flex_paged::lfit_page(r); }      // (paged_range.h: the read side's bound uses it too)

// the page size and the windows of a paged call, defaults resolved; false: not a legal combination
bool paged_params(uint32_t page_size, uint32_t& window_min, uint32_t& window_max) {
    if (page_size < 64u || page_size > (4u << 20)) return false;
    if (window_min == 0u) window_min = 4u * page_size;
    if (window_max == 0u) window_max = std::max(window_min, 65536u);
    return page_size <= window_min && window_min <= window_max && window_max <= 0x80000000u;
}

uint32_t paged_doublings(uint32_t window_min, uint32_t window_max) {
    uint32_t d = 0;
    for (uint64_t w = window_min; w < window_max; w *= 2u) d++;
    return d;
}

// max_rounds times the fit entry over the windows the step in front laid out in w, and the step behind it (lz4_paged.hip): the rounds of
// lz4flex_compress_paged behind its PAGED_FIRST step, and of lz4flex_paged_append behind its resume step
int paged_rounds(lz4flex_ctx* c, const PagedArgs& a, const PagedWork& w, const uint8_t* in_base, uint8_t* out_base, uint32_t max_rounds,
                 uint8_t* scratch, uint64_t scratch_cap, bool big, hipStream_t s) {
    const FitArgs round{nullptr, nullptr, nullptr, in_base, w.w_off, w.w_len, a.n, out_base, w.o_off, w.o_cap, w.r_len, w.r_used, w.r_st};
    for (uint32_t r = 0; r < max_rounds; r++) {
        if (const int rc = compress_fit_on_device(c, round, scratch, scratch_cap, w.packed, big, s)) return rc;
        const hipError_t e = launch_paged_step(a, w, r + 1u == max_rounds ? PAGED_LAST : PAGED_NEXT, s);
        if (e != hipSuccess) return hip_fail(e, "paged step launch");
    }
    return 0;
}

// the rounds of a paged call on device memory: the step (lz4_paged.hip), then max_rounds times the fit entry over the windows the
// step laid out and the step behind it.  a's arrays, in_base and out_base are device memory; nothing is allocated or synchronised.
int paged_on_device(lz4flex_ctx* c, const PagedArgs& a, const uint8_t* in_base, uint8_t* out_base, uint32_t max_rounds, uint8_t* scratch,
                    uint64_t scratch_cap, void* work, bool big, hipStream_t s) {
    const PagedWork w = paged_work(work, a.n);
    const hipError_t e = launch_paged_step(a, w, PAGED_FIRST | (max_rounds == 0u ? PAGED_LAST : 0), s);
    if (e != hipSuccess) return hip_fail(e, "paged step launch");
    return paged_rounds(c, a, w, in_base, out_base, max_rounds, scratch, scratch_cap, big, s);
}

struct PagedCall {
    const uint8_t* in_base; const uint64_t* in_off; const uint32_t* in_len; uint32_t n;
    uint32_t page_size, window_min, window_max, max_rounds;
    uint8_t* out_base; const uint64_t* page_off; uint32_t* page_len; uint32_t* page_src; uint32_t* n_pages; uint32_t* in_done; int32_t* status;
};

// MEM_HOST: the streams' span and the descriptors go up, the rounds the lengths can need run as on device memory, the tables, the
// results and the page file come down with one synchronisation; committed pages (their page_len bytes) and their table entries are
// copied to their places, the rest of the caller's page file and tables stays as it is.
int paged_on_host(lz4flex_ctx* c, const PagedCall& p, bool big) {
    const uint32_t n = p.n;
    DeviceGuard guard(c->device);
    HIP_TRY(guard.err);
    const Span in_span = span_of(p.in_off, p.in_len, n);
    const uint64_t first = p.page_off[0], entries = p.page_off[n] - first;
    const size_t out_bytes = (size_t)(entries * p.page_size);
    uint64_t slots = 0;
    uint32_t longest = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t w = std::min(p.in_len[i], p.window_max);
        slots += lz4flex_get_maximum_output_size(w);
        big = big || w > 65536u;
        longest = std::max(longest, p.in_len[i]);
    }
    const uint32_t rounds = std::min(p.max_rounds, lz4flex_paged_rounds_bound(longest, p.page_size, p.window_min, p.window_max));
    HostStage st;
    const auto in_off = st.up<uint64_t>(n), page_off = st.up<uint64_t>((size_t)n + 1u);
    const auto in_len = st.up<uint32_t>(n);
    const auto page_len = st.down<uint32_t>((size_t)entries), page_src = st.down<uint32_t>((size_t)entries);
    const auto n_pages = st.down<uint32_t>(n), in_done = st.down<uint32_t>(n);
    const auto status = st.down<int32_t>(n);
    const Region r_in = st.region(in_span.bytes(), 64), r_out = st.region(out_bytes, 64);
    st.columns();
    const Region r_work = st.region(paged_work_bytes(n), 0);
    int rc;
    if ((rc = stage_open(c, st))) return rc;
    if ((rc = ensure_buf(c->pay, out_bytes + 16))) return rc;
    void* d_scratch = nullptr;
    if ((rc = ctx_scratch(c, 0, (size_t)slots + 256, &d_scratch))) return rc;
    st.fill_offsets(in_off, p.in_off, in_span.lo); st.fill_offsets(page_off, p.page_off, first);
    st.fill(in_len, p.in_len);
    hipStream_t s = st.s;
    HIP_TRY(st.send(r_in, p.in_base + in_span.lo));
    HIP_TRY(st.send_columns());
    const PagedArgs dv{st.dev(in_off), st.dev(in_len), n, p.page_size, p.window_min, p.window_max, st.dev(page_off), st.dev_opt(page_len),
                       st.dev_opt(page_src), st.dev(n_pages), st.dev(in_done), st.dev(status)};
    if ((rc = paged_on_device(c, dv, st.dev(r_in), st.dev(r_out), rounds, (uint8_t*)d_scratch, slots, st.dev(r_work), big, s))) return rc;
    HIP_TRY(st.fetch_columns(page_len));
    if (out_bytes) HIP_TRY(hipMemcpyAsync(c->pay.p, st.dev(r_out), out_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    st.read(n_pages, p.n_pages); st.read(in_done, p.in_done); st.read(status, p.status);
    const uint32_t* h_len = st.host(page_len);
    const uint32_t* h_src = st.host(page_src);
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t k = 0; k < p.n_pages[i]; k++) {
            const uint64_t e = p.page_off[i] + k, r = e - first;
            p.page_len[e] = h_len[r]; p.page_src[e] = h_src[r];
            memcpy(p.out_base + e * p.page_size, c->pay.p + r * p.page_size, h_len[r]);
        }
    return 0;
}

}  // namespace

extern "C" {

uint64_t lz4flex_paged_pages_bound(uint32_t in_len, uint32_t page_size) {
    if (page_size < 64u || page_size > (4u << 20)) return 0;
    const uint64_t L = lfit_unbounded(page_size);
    return ((uint64_t)in_len + L - 1u) / L;
}

uint32_t lz4flex_paged_rounds_bound(uint32_t max_in_len, uint32_t page_size, uint32_t window_min, uint32_t window_max) {
    if (!paged_params(page_size, window_min, window_max)) return 0;
    return (uint32_t)(lz4flex_paged_pages_bound(max_in_len, page_size) + paged_doublings(window_min, window_max));
}

size_t lz4flex_compress_paged_work_size(uint32_t n) { return paged_work_bytes(n); }

int lz4flex_compress_paged(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len, uint32_t n, uint32_t page_size,
                           uint32_t window_min, uint32_t window_max, uint32_t max_rounds, void* out_base, const uint64_t* page_off,
                           uint32_t* page_len, uint32_t* page_src, uint32_t* n_pages, uint32_t* in_done, int32_t* status, void* scratch,
                           uint64_t scratch_cap, void* work, int mem_kind, void* hip_stream) {
    if (!paged_params(page_size, window_min, window_max)) return -LZ4FLEX_E_INVALID_ARG;
    const MemKind k = classify_mem(mem_kind, LZ4FLEX_MEM_BIG_BLOCKS, LZ4FLEX_MEM_BIG_BLOCKS);     // (no LZ4FLEX_MEM_CHAINED)
    if (k.where == Mem::Invalid) return -LZ4FLEX_E_INVALID_ARG;
    if (n == 0) return 0;
    if (!in_off || !in_len || !page_off || !page_len || !page_src || !n_pages || !in_done || !status) return -LZ4FLEX_E_INVALID_ARG;
    if (k.where == Mem::Device && (!work || !scratch)) return -LZ4FLEX_E_INVALID_ARG;
    if (k.where == Mem::Host)                                   // (the entries are visible: they count up)
        for (uint32_t i = 0; i < n; i++)
            if (page_off[i + 1] < page_off[i]) return -LZ4FLEX_E_INVALID_ARG;
    int rc;
    if ((rc = ctx_resolve(&ctx))) return rc;                  // (compress_batch_entry has the "debug_fail_next_batch" hook)
    if (k.where == Mem::Device) {
        const PagedArgs a{in_off, in_len, n, page_size, window_min, window_max, page_off, page_len, page_src, n_pages, in_done, status};
        return paged_on_device(ctx, a, (const uint8_t*)in_base, (uint8_t*)out_base, max_rounds, (uint8_t*)scratch, scratch_cap, work, k.big,
                               (hipStream_t)hip_stream);
    }
    const PagedCall p{(const uint8_t*)in_base, in_off, in_len, n, page_size, window_min, window_max, max_rounds, (uint8_t*)out_base, page_off,
                      page_len, page_src, n_pages, in_done, status};
    return paged_on_host(ctx, p, k.big);
}

// ---- paged streams, the read side: m byte ranges in one call, planned on the device (lz4_paged_read.hip) ------------------------------
}  // extern "C"

namespace {

using lz4flex_paged::RangeRec;

// a call on device memory: a fixed sequence of launches sized by m and max_items; nothing is allocated, read back or synchronised
int paged_read_on_device(lz4flex_ctx* c, const PagedReadArgs& a, const uint8_t* pages, uint8_t* out_base, uint8_t* scratch, void* work, bool big,
                         hipStream_t s) {
    const PagedReadWork w = paged_read_work(work, a.m, a.max_items);
    hipError_t e = launch_paged_read_locate(a, w, s);
    if (e == hipSuccess) e = launch_packed_scan(w.nb, a.m, 1u, ~0ull, 0u, w.tiles, w.slot, nullptr, nullptr, nullptr, s);
    if (e == hipSuccess) e = launch_packed_scan(w.hb, a.m, lz4flex_paged::HEAD_ALIGN, ~0ull, 0u, w.tiles, w.head_off, nullptr, nullptr, nullptr, s);
    if (e == hipSuccess) e = launch_paged_read_plan(a, w, s);
    if (e != hipSuccess) return hip_fail(e, "paged read plan launch");
    const int mem = LZ4FLEX_MEM_DEVICE | (big ? LZ4FLEX_MEM_BIG_BLOCKS : 0);
    int rc;
    if (a.max_items &&
        (rc = lz4flex_decompress_batch_partial(c, pages, w.a_in, w.a_len, a.max_items, out_base, w.a_out, w.a_tgt, w.a_olen, w.a_st, mem, s))) return rc;
    if (a.scratch_cap) {                                         // (no scratch: no range with a head is served, b_* is not read)
        if ((rc = lz4flex_decompress_batch_partial(c, pages, w.b_in, w.b_len, a.m, scratch, w.b_out, w.b_tgt, w.b_olen, w.b_st, mem, s))) return rc;
        e = launch_copy_batch(scratch, w.d_src, w.d_len, out_base, w.d_dst, a.m, s);
        if (e != hipSuccess) return hip_fail(e, "paged read gather launch");
    }
    e = launch_paged_read_verdict(a, w, s);
    return e != hipSuccess ? hip_fail(e, "paged read verdict launch") : 0;
}

struct PagedReadCall {
    const uint8_t* pages; lz4flex_paged::Tables t;
    const uint32_t* range_stream; const uint32_t* range_off; const uint32_t* range_len; uint32_t m;
    uint8_t* out_base; const uint64_t* out_off; uint32_t* out_len; int32_t* status;
};

// One MEM_HOST pass: the ranges live[0 .. R) (located, sound, E touched pages in all) become R streams of a table of their own -- stream
// q holds range q's touched pages and ends where its last page does --, the span of every range's pages goes up, the device path runs
// with exactly the items and the scratch the pass needs, the results and the output come down with one synchronisation.
int paged_read_pass(lz4flex_ctx* c, const PagedReadCall& p, const RangeRec* recs, const uint32_t* live, uint32_t R, uint64_t E, bool big) {
    const uint32_t P = p.t.page_size;
    uint64_t out_bytes = 0, head_bytes = 0;
    for (uint32_t q = 0; q < R; q++) {
        out_bytes += align_up(recs[live[q]].len, 64);
        head_bytes += lz4flex_paged::head_slot_bytes(recs[live[q]]);
    }
    HostStage st;
    const auto page_off = st.up<uint64_t>((size_t)R + 1u), out_off = st.up<uint64_t>(R);
    const auto page_len = st.up<uint32_t>((size_t)E), page_src = st.up<uint32_t>((size_t)E);
    const auto n_pages = st.up<uint32_t>(R), in_done = st.up<uint32_t>(R), r_stream = st.up<uint32_t>(R), r_off = st.up<uint32_t>(R), r_len = st.up<uint32_t>(R);
    const auto out_len = st.down<uint32_t>(R);
    const auto status = st.down<int32_t>(R);
    const Region r_in = st.region((size_t)(E * P), 64), r_out = st.region((size_t)out_bytes, 64), r_heads = st.region((size_t)head_bytes, 64);
    st.columns();
    const Region r_work = st.region(paged_read_work_bytes(R, (uint32_t)E), 0);
    int rc;
    if ((rc = stage_open(c, st))) return rc;
    if ((rc = ensure_buf(c->pay, (size_t)out_bytes + 16))) return rc;
    hipStream_t s = st.s;
    uint64_t e_at = 0, o_at = 0;
    for (uint32_t q = 0; q < R; q++) {
        const RangeRec& r = recs[live[q]];
        const uint64_t e0 = r.first + r.j0;
        const uint32_t j1 = r.j0 + r.nb - 1u;
        st.host(page_off)[q] = e_at; st.host(out_off)[q] = o_at;
        memcpy(st.host(page_len) + e_at, p.t.page_len + e0, 4ull * r.nb);
        memcpy(st.host(page_src) + e_at, p.t.page_src + e0, 4ull * r.nb);
        st.host(n_pages)[q] = r.nb;
        st.host(in_done)[q] = j1 + 1u < r.k ? p.t.page_src[r.first + j1 + 1u] : r.S;
        st.host(r_stream)[q] = q; st.host(r_off)[q] = r.off; st.host(r_len)[q] = r.len;
        HIP_TRY(hipMemcpyAsync(st.dev(r_in) + e_at * P, p.pages + e0 * P, (size_t)r.nb * P, hipMemcpyHostToDevice, s));
        e_at += r.nb; o_at += align_up(r.len, 64);
    }
    st.host(page_off)[R] = e_at;
    HIP_TRY(st.send_columns());
    PagedReadArgs dv{};
    dv.t = lz4flex_paged::Tables{st.dev(page_off), st.dev(page_len), st.dev(page_src), st.dev(n_pages), st.dev(in_done), R, P};
    dv.range_stream = st.dev(r_stream); dv.range_off = st.dev(r_off); dv.range_len = st.dev(r_len); dv.m = R;
    dv.out_off = st.dev(out_off); dv.out_len = st.dev(out_len); dv.status = st.dev(status);
    dv.max_items = (uint32_t)E; dv.scratch_cap = head_bytes;
    if ((rc = paged_read_on_device(c, dv, st.dev(r_in), st.dev(r_out), st.dev(r_heads), st.dev(r_work), big, s))) return rc;
    HIP_TRY(st.fetch_columns(out_len));
    if (out_bytes) HIP_TRY(hipMemcpyAsync(c->pay.p, st.dev(r_out), (size_t)out_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint32_t q = 0; q < R; q++) {
        const uint32_t r = live[q];
        p.status[r] = st.host(status)[q]; p.out_len[r] = st.host(out_len)[q];
        if (p.status[r] == 0 && p.out_len[r]) memcpy(p.out_base + p.out_off[r], c->pay.p + st.host(out_off)[q], p.out_len[r]);
    }
    return 0;
}

// MEM_HOST: the host locates the ranges itself (paged_range.h, the functions the kernels run) and answers the ranges that need no
// device -- no such stream, nothing wanted, a contradicting table; the others go up in passes of at most "frame_range_pass_bytes" of
// staging (a pass takes at least one range).
int paged_read_on_host(lz4flex_ctx* c, const PagedReadCall& p, bool big) {
    DeviceGuard guard(c->device);
    HIP_TRY(guard.err);
    std::vector<RangeRec> recs(p.m);
    std::vector<uint32_t> live;
    for (uint32_t r = 0; r < p.m; r++) {
        RangeRec& q = recs[r];
        lz4flex_paged::locate(p.t, p.range_stream[r], p.range_off[r], p.range_len[r], &q);
        p.out_len[r] = 0u;
        if (q.flags & lz4flex_paged::REC_NO_STREAM) { p.status[r] = LZ4FLEX_E_INVALID_ARG; continue; }
        if (q.len == 0u) { p.status[r] = 0; continue; }
        bool ok = (q.flags & lz4flex_paged::REC_BAD) == 0u;
        for (uint32_t j = 0; ok && j < q.nb; j++) ok = lz4flex_paged::page_ok(p.t, q, q.j0 + j);
        if (!ok) { p.status[r] = LZ4FLEX_E_INVALID_ARG; continue; }
        live.push_back(r);
    }
    const uint64_t pass_bytes = (uint64_t)std::max(c->range_pass_bytes, 1);
    for (size_t first = 0; first < live.size();) {
        uint64_t bytes = 0, E = 0;
        size_t i = first;
        for (; i < live.size(); i++) {
            const RangeRec& q = recs[live[i]];
            const uint64_t cost = (uint64_t)q.nb * p.t.page_size + align_up(q.len, 64) + lz4flex_paged::head_slot_bytes(q);
            if (i > first && (cost > pass_bytes - std::min(bytes, pass_bytes) || E + q.nb > 0x7FFFFFFFull)) break;
            bytes += cost; E += q.nb;
        }
        if (E > 0xFFFFFFFFull) return -LZ4FLEX_E_UNSUPPORTED;
        if (const int rc = paged_read_pass(c, p, recs.data(), live.data() + first, (uint32_t)(i - first), E, big)) return rc;
        first = i;
    }
    return 0;
}

}  // namespace

extern "C" {

uint32_t lz4flex_paged_range_pages_bound(uint32_t range_len, uint32_t page_size) { return lz4flex_paged::pages_bound(range_len, page_size); }

size_t lz4flex_paged_read_work_size(uint32_t m, uint32_t max_items) { return paged_read_work_bytes(m, max_items); }

int lz4flex_paged_read_ranges(lz4flex_ctx* ctx, const void* pages, uint32_t page_size, const uint64_t* page_off, const uint32_t* page_len,
                              const uint32_t* page_src, const uint32_t* n_pages, const uint32_t* in_done, uint32_t n, const uint32_t* range_stream,
                              const uint32_t* range_off, const uint32_t* range_len, uint32_t m, void* out_base, const uint64_t* out_off,
                              uint32_t* out_len, int32_t* status, uint32_t max_items, void* scratch, uint64_t scratch_cap, void* work, int mem_kind,
                              void* hip_stream) {
    const MemKind k = classify_mem(mem_kind, LZ4FLEX_MEM_BIG_BLOCKS, LZ4FLEX_MEM_BIG_BLOCKS);     // (no LZ4FLEX_MEM_CHAINED)
    if (k.where == Mem::Invalid) return -LZ4FLEX_E_INVALID_ARG;
    if (page_size < lz4flex_paged::PAGE_MIN || page_size > lz4flex_paged::PAGE_MAX) return -LZ4FLEX_E_INVALID_ARG;
    if (m == 0) return 0;
    if (!page_off || !page_len || !page_src || !n_pages || !in_done || !range_stream || !range_off || !range_len || !out_off || !out_len || !status)
        return -LZ4FLEX_E_INVALID_ARG;
    if (k.where == Mem::Device && (!work || (!scratch && scratch_cap))) return -LZ4FLEX_E_INVALID_ARG;
    int rc;
    if ((rc = ctx_resolve(&ctx))) return rc;                  // (lz4flex_decompress_batch_partial has the "debug_fail_next_batch" hook)
    const lz4flex_paged::Tables t{page_off, page_len, page_src, n_pages, in_done, n, page_size};
    if (k.where == Mem::Device) {
        const PagedReadArgs a{t, range_stream, range_off, range_len, m, out_off, out_len, status, max_items, scratch_cap};
        return paged_read_on_device(ctx, a, (const uint8_t*)pages, (uint8_t*)out_base, (uint8_t*)scratch, work, k.big, (hipStream_t)hip_stream);
    }
    const PagedReadCall p{(const uint8_t*)pages, t, range_stream, range_off, range_len, m, (uint8_t*)out_base, out_off, out_len, status};
    try {
        return paged_read_on_host(ctx, p, k.big || page_size > 131072u);
    } catch (...) { return -LZ4FLEX_E_NOMEM; }
}

// ---- paged streams, append: new bytes for any subset of the streams, the tail page reopened (lz4_paged_append.hip, paged_append.h) ----
}  // extern "C"

namespace {

using lz4flex_paged::AppendRec;

// a call on device memory: a fixed sequence of launches sized by n and max_rounds; nothing is allocated, read back or synchronised
int paged_append_on_device(lz4flex_ctx* c, const PagedAppendArgs& a, const uint8_t* add_base, uint8_t* pages, uint8_t* stage, uint32_t max_rounds,
                           uint8_t* scratch, uint64_t scratch_cap, void* work, bool big, bool big_pages, hipStream_t s) {
    const PagedAppendWork w = paged_append_work(work, a.n);
    hipError_t e = launch_paged_append_locate(a, w, s);
    if (e == hipSuccess) e = launch_packed_scan(w.need, a.n, 1u, ~0ull, 0u, w.tiles, w.slot, nullptr, nullptr, nullptr, s);
    if (e == hipSuccess) e = launch_paged_append_emit(a, w, s);
    if (e != hipSuccess) return hip_fail(e, "paged append plan launch");
    const int mem = LZ4FLEX_MEM_DEVICE | (big_pages ? LZ4FLEX_MEM_BIG_BLOCKS : 0);
    if (const int rc = lz4flex_decompress_batch_partial(c, pages, w.t_in, w.t_len, a.n, stage, w.t_out, w.t_tgt, w.t_olen, w.t_st, mem, s)) return rc;
    e = launch_copy_batch(add_base, w.c_src, w.c_len, stage, w.c_dst, a.n, s);
    if (e == hipSuccess) e = launch_paged_append_resume(a, w, max_rounds == 0u, s);
    if (e != hipSuccess) return hip_fail(e, "paged append resume launch");
    const PagedArgs rounds{w.v_off, w.v_len, a.n, a.page_size, a.window_min, a.window_max, a.page_off, a.page_len, a.page_src, a.n_pages, a.in_done,
                           a.status};
    return paged_rounds(c, rounds, paged_work(w.paged, a.n), stage, pages, max_rounds, scratch, scratch_cap, big, s);
}

struct PagedAppendCall {
    const uint8_t* add_base; const uint64_t* add_off; const uint32_t* add_len; uint32_t n;
    uint32_t page_size, window_min, window_max, max_rounds;
    uint8_t* pages; const uint64_t* page_off; uint32_t* page_len; uint32_t* page_src; uint32_t* n_pages; uint32_t* in_done; int32_t* status;
    uint64_t* stage_off; uint32_t* tail_src;
};

// MEM_HOST: the host runs steps 1 to 3 itself (paged_append.h, the functions the kernels run) and answers the streams that take no part
// or whose table contradicts itself; the others become the streams of a table of their own -- stream i holds its reopened entry and the
// free entries behind it, a stream that does not go on holds none and has nothing to add, so n is the caller's in every round -- whose
// tail pages and new bytes go up.  The device path runs with exactly the stage it needs, the entries and pages from the reopened one on
// -- as many as T + A bytes can take, not the room the caller keeps behind them -- and the results come down with one synchronisation and
// are copied to their places.
int paged_append_on_host(lz4flex_ctx* c, const PagedAppendCall& p, bool big) {
    const uint32_t n = p.n, P = p.page_size;
    DeviceGuard guard(c->device);
    HIP_TRY(guard.err);
    const lz4flex_paged::AppendTables t{p.page_off, p.page_len, p.page_src, p.n_pages, p.in_done, n, P, p.window_max};
    std::vector<AppendRec> recs(n);
    std::vector<uint8_t> go(n);
    Span add_span;
    // the entries stream i gets in the device's table: the reopened one and the free ones behind it, and no more than T + A bytes can
    // take (the pages bound) -- what goes up, is reserved and comes down follows the new bytes, not the room the caller keeps
    const auto room_of = [&](const AppendRec& q) {
        return std::min<uint64_t>(lz4flex_paged::append_room(q), lz4flex_paged_pages_bound(q.T + q.A, P));
    };
    uint64_t entries = 0, stage_bytes = 0, slots = 0;
    uint32_t longest = 0, going = 0;
    for (uint32_t i = 0; i < n; i++) {
        AppendRec& q = recs[i];
        lz4flex_paged::append_locate(t, i, p.add_len[i], &q);
        const int32_t pre = lz4flex_paged::append_pre(q, 0, ~0ull);
        go[i] = pre == -1;
        p.stage_off[i] = lz4flex_paged::NO_STAGE;
        p.tail_src[i] = go[i] ? q.base : q.S;
        if (!go[i]) {                                         // (a dead stream still has an empty window in every round: its scratch slot)
            p.status[i] = pre;
            slots += lz4flex_get_maximum_output_size(0);
            continue;
        }
        const uint64_t room = room_of(q);
        if (entries + room > 0xFFFFFFFFull) return -LZ4FLEX_E_UNSUPPORTED;
        entries += room; going++;
        stage_bytes += lz4flex_paged::append_slot_bytes(q);
        const uint32_t v = q.T + q.A, w = std::min(v, p.window_max);
        slots += lz4flex_get_maximum_output_size(w);
        big = big || w > 65536u;
        longest = std::max(longest, v);
        add_span.add(p.add_off[i], q.A);
    }
    if (going == 0u) return 0;
    add_span = add_span.closed();
    const uint32_t rounds = std::min(p.max_rounds, lz4flex_paged_rounds_bound(longest, P, p.window_min, p.window_max));
    const size_t out_bytes = (size_t)(entries * P);
    HostStage st;
    const auto add_off = st.up<uint64_t>(n), page_off = st.up<uint64_t>((size_t)n + 1u);
    const auto add_len = st.up<uint32_t>(n);
    const auto page_len = st.up<uint32_t>((size_t)entries), page_src = st.up<uint32_t>((size_t)entries);       // (these four go up and come down)
    const auto n_pages = st.up<uint32_t>(n), in_done = st.up<uint32_t>(n);
    const auto status = st.down<int32_t>(n);
    const auto stage_off = st.down<uint64_t>(n);
    const auto tail_src = st.down<uint32_t>(n);
    const Region r_add = st.region(add_span.bytes(), 64), r_out = st.region(out_bytes, 64), r_stage = st.region((size_t)stage_bytes, 64);
    st.columns();
    const Region r_work = st.region(paged_append_work_bytes(n), 0);
    int rc;
    if ((rc = stage_open(c, st))) return rc;
    if ((rc = ensure_buf(c->pay, out_bytes + 16))) return rc;
    void* d_scratch = nullptr;
    if ((rc = ctx_scratch(c, 0, (size_t)slots + 256, &d_scratch))) return rc;
    hipStream_t s = st.s;
    st.zero(page_len); st.zero(page_src);
    uint64_t e_at = 0;
    for (uint32_t i = 0; i < n; i++) {
        const AppendRec& q = recs[i];
        st.host(page_off)[i] = e_at;
        st.host(add_off)[i] = go[i] ? p.add_off[i] - add_span.lo : 0ull;
        st.host(add_len)[i] = go[i] ? q.A : 0u;
        st.host(n_pages)[i] = go[i] && q.k != 0u ? 1u : 0u;
        st.host(in_done)[i] = go[i] ? q.S : 0u;
        if (!go[i]) continue;
        if (q.k != 0u) {
            const uint64_t e = q.first + (q.k - 1u);
            st.host(page_len)[e_at] = p.page_len[e]; st.host(page_src)[e_at] = p.page_src[e];
            HIP_TRY(hipMemcpyAsync(st.dev(r_out) + e_at * P, p.pages + e * P, p.page_len[e], hipMemcpyHostToDevice, s));
        }
        e_at += room_of(q);
    }
    st.host(page_off)[n] = e_at;
    HIP_TRY(st.send(r_add, p.add_base + add_span.lo));
    HIP_TRY(st.send_columns());
    const PagedAppendArgs dv{st.dev(add_off), st.dev(add_len), n, P, p.window_min, p.window_max, st.dev(page_off), st.dev_opt(page_len),
                             st.dev_opt(page_src), st.dev(n_pages), st.dev(in_done), st.dev(status), stage_bytes, st.dev(stage_off), st.dev(tail_src)};
    if ((rc = paged_append_on_device(c, dv, st.dev(r_add), st.dev(r_out), st.dev(r_stage), rounds, (uint8_t*)d_scratch, slots, st.dev(r_work),
                                     big, big || P > 131072u, s)))
        return rc;
    std::vector<uint32_t> resumed(n);                         // (v_len: S + A where the rounds took the stream's tables over, else 0)
    HIP_TRY(hipMemcpyAsync(resumed.data(), paged_append_work(st.dev(r_work), n).v_len, 4ull * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(st.fetch_columns(page_len));
    if (out_bytes) HIP_TRY(hipMemcpyAsync(c->pay.p, st.dev(r_out), out_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t* h_len = st.host(page_len);
    const uint32_t* h_src = st.host(page_src);
    for (uint32_t i = 0; i < n; i++) {
        if (!go[i]) continue;
        const AppendRec& q = recs[i];
        p.status[i] = st.host(status)[i];
        p.tail_src[i] = st.host(tail_src)[i];
        const uint32_t k0 = lz4flex_paged::append_k0(q), got = st.host(n_pages)[i];
        if (resumed[i] == 0u) continue;                       // (the tail page did not deliver: the stream is untouched)
        p.n_pages[i] = k0 + got; p.in_done[i] = st.host(in_done)[i];
        for (uint32_t j = 0; j < got; j++) {
            const uint64_t e = q.first + k0 + j, r = st.host(page_off)[i] + j;
            p.page_len[e] = h_len[r]; p.page_src[e] = h_src[r];
            memcpy(p.pages + e * P, c->pay.p + r * P, h_len[r]);
        }
    }
    return 0;
}

}  // namespace

extern "C" {

size_t lz4flex_paged_append_work_size(uint32_t n) { return paged_append_work_bytes(n); }

uint64_t lz4flex_paged_append_stage_bound(uint64_t sum_add_len, uint32_t n, uint32_t window_max) {
    if (window_max == 0u) window_max = 65536u;
    if (window_max < lz4flex_paged::PAGE_MIN || window_max > 0x80000000u) return 0;
    return lz4flex_paged::append_stage_bound(sum_add_len, n, window_max);
}

int lz4flex_paged_append(lz4flex_ctx* ctx, const void* add_base, const uint64_t* add_off, const uint32_t* add_len, uint32_t n, uint32_t page_size,
                         uint32_t window_min, uint32_t window_max, uint32_t max_rounds, void* pages, const uint64_t* page_off, uint32_t* page_len,
                         uint32_t* page_src, uint32_t* n_pages, uint32_t* in_done, int32_t* status, void* stage, uint64_t stage_cap,
                         uint64_t* stage_off, uint32_t* tail_src, void* scratch, uint64_t scratch_cap, void* work, int mem_kind, void* hip_stream) {
    if (!paged_params(page_size, window_min, window_max)) return -LZ4FLEX_E_INVALID_ARG;
    const MemKind k = classify_mem(mem_kind, LZ4FLEX_MEM_BIG_BLOCKS, LZ4FLEX_MEM_BIG_BLOCKS);     // (no LZ4FLEX_MEM_CHAINED)
    if (k.where == Mem::Invalid) return -LZ4FLEX_E_INVALID_ARG;
    if (n == 0) return 0;
    if (!add_off || !add_len || !page_off || !page_len || !page_src || !n_pages || !in_done || !status || !stage_off || !tail_src)
        return -LZ4FLEX_E_INVALID_ARG;
    if (k.where == Mem::Device && (!work || !scratch || !stage)) return -LZ4FLEX_E_INVALID_ARG;
    int rc;
    if ((rc = ctx_resolve(&ctx))) return rc;                  // (lz4flex_decompress_batch_partial has the "debug_fail_next_batch" hook)
    if (k.where == Mem::Device) {
        const PagedAppendArgs a{add_off, add_len, n, page_size, window_min, window_max, page_off, page_len, page_src, n_pages, in_done, status,
                                stage_cap, stage_off, tail_src};
        return paged_append_on_device(ctx, a, (const uint8_t*)add_base, (uint8_t*)pages, (uint8_t*)stage, max_rounds, (uint8_t*)scratch, scratch_cap,
                                      work, k.big, k.big, (hipStream_t)hip_stream);
    }
    const PagedAppendCall p{(const uint8_t*)add_base, add_off, add_len, n, page_size, window_min, window_max, max_rounds, (uint8_t*)pages, page_off,
                            page_len, page_src, n_pages, in_done, status, stage_off, tail_src};
    try {
        return paged_append_on_host(ctx, p, k.big);
    } catch (...) { return -LZ4FLEX_E_NOMEM; }
}

// ---- scalar, lz4_flex-shaped: 1-block host batches ------------------------------------------
static const uint64_t OFF0 = 0;
static const uint8_t EMPTY = 0;

int64_t lz4flex_compress_into(const uint8_t* in, size_t in_len, uint8_t* out, size_t out_cap) {
    if (in_len > 0xFFFFFFFFull) return -LZ4FLEX_E_INVALID_ARG;
    // compress.rs:338-340: OutputTooSmall is decided up front, before anything is written
    if (out_cap < lz4flex_get_maximum_output_size(in_len)) return -LZ4FLEX_E_OUTPUT_TOO_SMALL;
    lz4flex_ctx* c;
    int rc = default_ctx(&c);
    if (rc) return rc;
    const uint32_t len = (uint32_t)in_len, cap = (uint32_t)std::min<size_t>(out_cap, 0xFFFFFFFFull);
    uint32_t olen = 0;
    int32_t st = 0;
    const BatchCall b = batch_of(true, in ? in : &EMPTY, &OFF0, &len, 1, out, &OFF0, &cap, &olen, &st);
    rc = run_host_batch(c, b);
    if (rc) return rc;
    if (st) return -(int64_t)st;
    return (int64_t)olen;
}

int lz4flex_compress_chains(lz4flex_ctx* ctx, const void* in_base, const lz4flex_chain_block* blocks, uint32_t n_blocks,
                            const uint32_t* chain_first, const uint32_t* chain_count, uint32_t n_chains, void* out_base,
                            const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len, int32_t* status,
                            uint32_t* tbl_state, int mem_kind, void* hip_stream) {
    static_assert(sizeof(lz4flex_chain_block) == 40, "ChainBlock layout");
    int rc;
    if ((rc = ctx_resolve(&ctx))) return rc;
    if (n_chains == 0 || n_blocks == 0) return 0;
    if (!blocks || !chain_first || !chain_count || !out_off || !out_cap || !out_len || !status) return -LZ4FLEX_E_INVALID_ARG;
    const MemKind k = classify_mem(mem_kind, 0, ANY_FLAGS);
    if (k.where == Mem::Device) {
        hipError_t le = launch_compress_chain((const uint8_t*)in_base, blocks, chain_first, chain_count, n_chains,
                                              (uint8_t*)out_base, out_off, out_cap, out_len, status, tbl_state,
                                              (hipStream_t)hip_stream);
        return le == hipSuccess ? 0 : hip_fail(le, "chain kernel launch");
    }
    if (k.where != Mem::Host) return -LZ4FLEX_E_INVALID_ARG;
    for (uint32_t i = 0; i < n_chains; i++)                     // host arrays can be checked: a chain stays inside `blocks`
        if (chain_first[i] > n_blocks || chain_count[i] > n_blocks - chain_first[i]) return -LZ4FLEX_E_INVALID_ARG;
    lz4flex_ctx* c = ctx;
    DeviceGuard guard(c->device);
    HIP_TRY(guard.err);
    // spans of the caller's buffers (a block's dictionary lies in the input buffer too)
    Span is;
    for (uint32_t i = 0; i < n_blocks; i++) {
        is.add(blocks[i].in_off, blocks[i].in_len);
        if (blocks[i].dict_len) is.add(blocks[i].dict_off, blocks[i].dict_len);
    }
    is = is.closed();
    const Span os = span_of(out_off, out_cap, n_blocks);
    HostStage st;
    const auto c_blocks = st.up<lz4flex_chain_block>(n_blocks);
    const auto c_first = st.up<uint32_t>(n_chains), c_count = st.up<uint32_t>(n_chains);
    const auto c_out_off = st.up<uint64_t>(n_blocks);
    const auto c_out_cap = st.up<uint32_t>(n_blocks);
    const auto c_out_len = st.down<uint32_t>(n_blocks);
    const auto c_status = st.down<int32_t>(n_blocks);
    const Region r_in = st.region(is.bytes(), 64), r_out = st.region(os.bytes(), 64);
    st.columns(64);
    const Region r_tbl = st.region(tbl_state ? 16384ull * n_chains : 0, 0);
    if ((rc = stage_open(c, st))) return rc;
    lz4flex_chain_block* hb = st.host(c_blocks);
    for (uint32_t i = 0; i < n_blocks; i++) {
        hb[i] = blocks[i];
        hb[i].in_off -= is.lo;
        hb[i].dict_off = blocks[i].dict_len ? blocks[i].dict_off - is.lo : 0;
    }
    st.fill(c_first, chain_first); st.fill(c_count, chain_count);
    st.fill_offsets(c_out_off, out_off, os.lo); st.fill(c_out_cap, out_cap);
    hipStream_t s = st.s;
    HIP_TRY(st.send(r_in, (const uint8_t*)in_base + is.lo));
    HIP_TRY(st.send_columns());
    HIP_TRY(st.send(r_tbl, tbl_state));
    hipError_t le = launch_compress_chain(st.dev(r_in), st.dev(c_blocks), st.dev(c_first), st.dev(c_count), n_chains, st.dev(r_out), st.dev(c_out_off),
                                          st.dev(c_out_cap), st.dev(c_out_len), st.dev(c_status), tbl_state ? (uint32_t*)st.dev(r_tbl) : nullptr, s);
    if (le != hipSuccess) return hip_fail(le, "chain kernel launch");
    HIP_TRY(st.fetch_columns(c_out_len));
    if (tbl_state) HIP_TRY(hipMemcpyAsync(tbl_state, st.dev(r_tbl), r_tbl.bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    st.read(c_out_len, out_len); st.read(c_status, status);
    for (uint32_t i = 0; i < n_blocks; i++)
        if (status[i] == 0 && out_len[i])
            HIP_TRY(hipMemcpyAsync((uint8_t*)out_base + out_off[i], st.dev(r_out) + (out_off[i] - os.lo), out_len[i], hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int64_t lz4flex_compress_into_with_dict(const uint8_t* in, size_t in_len, uint8_t* out, size_t out_cap,
                                        const uint8_t* dict, size_t dict_len) {
    if (in_len > 0x7FFFFFFFull) return -LZ4FLEX_E_INVALID_ARG;
    if (out_cap < lz4flex_get_maximum_output_size(in_len)) return -LZ4FLEX_E_OUTPUT_TOO_SMALL;   // compress.rs:338-340
    {
        // "compress_mode" 2 with "compress_high_dict" 1: the high encoder's dictionary form, as a batch of one (it reads the
        // dictionary's last 32 KiB); every other setting: the reference's bytes below
        lz4flex_ctx* c = nullptr;
        if (default_ctx(&c) == 0 && c->comp_mode == 2 && c->comp_high_dict) {
            if (dict_len > 65536u) { dict += dict_len - 65536u; dict_len = 65536u; }
            const uint32_t len = (uint32_t)in_len, cap = (uint32_t)std::min<size_t>(out_cap, 0xFFFFFFFFull), dlen = (uint32_t)dict_len;
            uint32_t olen = 0;
            int32_t st = 0;
            BatchCall b = batch_of(true, in ? in : &EMPTY, &OFF0, &len, 1, out, &OFF0, &cap, &olen, &st);
            b.has_ext = true; b.dict_base = dict ? dict : &EMPTY; b.dict_off = &OFF0; b.dict_len = &dlen;
            const int rc = run_host_batch(c, b);
            if (rc) return rc;
            if (st) return -(int64_t)st;
            return (int64_t)olen;
        }
    }
    // compress_into_sink_with_dict, compress.rs:554-568, as a one-block chain (dict_chain_record): the staging buffer holds the
    // dictionary's last 64 KiB and the input behind them
    const size_t kept = std::min<size_t>(dict_len, 65536u);
    std::vector<uint8_t> buf(kept + in_len + 16);
    if (kept) memcpy(buf.data(), dict + (dict_len - kept), kept);
    if (in_len) memcpy(buf.data() + kept, in, in_len);
    const lz4flex_chain_block b = dict_chain_record<lz4flex_chain_block>(kept, (uint32_t)in_len, kept, dict_len);
    const uint32_t first = 0, count = 1;
    const uint32_t cap = (uint32_t)std::min<size_t>(out_cap, 0xFFFFFFFFull);
    uint32_t olen = 0;
    int32_t st = 0;
    int rc = lz4flex_compress_chains(nullptr, buf.data(), &b, 1, &first, &count, 1, out, &OFF0, &cap, &olen, &st, nullptr,
                                     LZ4FLEX_MEM_HOST, nullptr);
    if (rc) return rc;
    if (st) return -(int64_t)st;
    return (int64_t)olen;
}

int64_t lz4flex_compress_prepend_size(const uint8_t* in, size_t in_len, uint8_t* out, size_t out_cap) {
    // compress.rs:624-634: 4-byte LE length, then the block
    if (in_len > 0xFFFFFFFFull) return -LZ4FLEX_E_INVALID_ARG;   // (nothing is written before the arguments are known to be fine)
    if (out_cap < 4 || out_cap - 4 < lz4flex_get_maximum_output_size(in_len)) return -LZ4FLEX_E_OUTPUT_TOO_SMALL;
    const uint32_t n = (uint32_t)in_len;
    out[0] = (uint8_t)n; out[1] = (uint8_t)(n >> 8); out[2] = (uint8_t)(n >> 16); out[3] = (uint8_t)(n >> 24);
    int64_t r = lz4flex_compress_into(in, in_len, out + 4, out_cap - 4);
    return r < 0 ? r : r + 4;
}

static int64_t decompress_common(const uint8_t* in, size_t in_len, uint8_t* out, size_t out_cap, const uint8_t* dict,
                                 size_t dict_len, bool use_dict, lz4flex_err_detail* detail) {
    if (in_len > 0xFFFFFFFFull || out_cap > 0xFFFFFFFFull || dict_len > 0xFFFFFFFFull) return -LZ4FLEX_E_INVALID_ARG;
    if (detail) memset(detail, 0, sizeof *detail);
    lz4flex_ctx* c;
    int rc = default_ctx(&c);
    if (rc) { if (detail) detail->hip_error = g_last_hip; return rc; }
    const uint32_t len = (uint32_t)in_len, cap = (uint32_t)out_cap, dlen = (uint32_t)dict_len;
    uint32_t olen = 0;
    int32_t st = 0;
    uint64_t det[2] = {0, 0};
    static uint8_t sink_dummy = 0;
    BatchCall b = batch_of(false, in ? in : &EMPTY, &OFF0, &len, 1, out ? out : &sink_dummy, &OFF0, &cap, &olen, &st);
    b.detail = det;
    if (use_dict) { b.has_ext = true; b.dict_base = dict ? dict : &EMPTY; b.dict_off = &OFF0; b.dict_len = &dlen; }
    rc = run_host_batch(c, b);
    if (rc) { if (detail) detail->hip_error = g_last_hip; return rc; }
    if (st) {
        if (detail) { detail->expected = det[0]; detail->actual = det[1]; }
        return -(int64_t)st;
    }
    return (int64_t)olen;
}

int64_t lz4flex_decompress_into(const uint8_t* in, size_t in_len, uint8_t* out, size_t out_cap,
                                lz4flex_err_detail* detail) {
    return decompress_common(in, in_len, out, out_cap, nullptr, 0, false, detail);
}

int64_t lz4flex_decompress_into_with_dict(const uint8_t* in, size_t in_len, uint8_t* out, size_t out_cap,
                                          const uint8_t* dict, size_t dict_len, lz4flex_err_detail* detail) {
    return decompress_common(in, in_len, out, out_cap, dict, dict_len, true, detail);
}

// a one-block host batch of lz4flex_decompress_batch_partial (no OutputTooSmall: of `detail`, hip_error alone can be set)
int64_t lz4flex_decompress_partial_into(const uint8_t* in, size_t in_len, uint8_t* out, size_t target, lz4flex_err_detail* detail) {
    if (in_len > 0xFFFFFFFFull || target > 0xFFFFFFFFull) return -LZ4FLEX_E_INVALID_ARG;
    if (detail) memset(detail, 0, sizeof *detail);
    lz4flex_ctx* c;
    int rc = default_ctx(&c);
    if (rc) { if (detail) detail->hip_error = g_last_hip; return rc; }
    const uint32_t len = (uint32_t)in_len, want = (uint32_t)target;
    uint32_t olen = 0;
    int32_t st = 0;
    static uint8_t sink_dummy = 0;
    BatchCall b = batch_of(false, in ? in : &EMPTY, &OFF0, &len, 1, out ? out : &sink_dummy, &OFF0, &want, &olen, &st);
    b.partial = true;
    rc = run_host_batch(c, b);
    if (rc) { if (detail) detail->hip_error = g_last_hip; return rc; }
    return st ? -(int64_t)st : (int64_t)olen;
}

// a one-block host batch of lz4flex_decompress_batch_partial_shared_dict (no dictionary: of lz4flex_decompress_batch_partial)
int64_t lz4flex_decompress_partial_into_with_dict(const uint8_t* in, size_t in_len, uint8_t* out, size_t target, const uint8_t* dict, size_t dict_len,
                                                  lz4flex_err_detail* detail) {
    if (in_len > 0xFFFFFFFFull || target > 0xFFFFFFFFull || dict_len > 0xFFFFFFFFull || (!dict && dict_len)) return -LZ4FLEX_E_INVALID_ARG;
    if (!dict || !dict_len) return lz4flex_decompress_partial_into(in, in_len, out, target, detail);
    if (detail) memset(detail, 0, sizeof *detail);
    lz4flex_ctx* c;
    int rc = default_ctx(&c);
    if (rc) { if (detail) detail->hip_error = g_last_hip; return rc; }
    const uint32_t len = (uint32_t)in_len, want = (uint32_t)target;
    uint32_t olen = 0;
    int32_t st = 0;
    static uint8_t sink_dummy = 0;
    BatchCall b = batch_of(false, in ? in : &EMPTY, &OFF0, &len, 1, out ? out : &sink_dummy, &OFF0, &want, &olen, &st);
    b.partial = true; b.has_ext = true; b.shared_dict = dict; b.shared_len = (uint32_t)dict_len;
    rc = run_host_batch(c, b);
    if (rc) { if (detail) detail->hip_error = g_last_hip; return rc; }
    return st ? -(int64_t)st : (int64_t)olen;
}

int lz4flex_xxh32_batch_device(const void* base, const uint64_t* off, const uint32_t* len, uint32_t n, uint32_t seed,
                               uint32_t* out, void* hip_stream) {
    if (n && (!base || !off || !len || !out)) return -LZ4FLEX_E_INVALID_ARG;
    hipError_t le = launch_xxh32_batch((const uint8_t*)base, off, len, n, seed, out, (hipStream_t)hip_stream);
    return le == hipSuccess ? 0 : hip_fail(le, "xxh32 kernel launch");
}

int lz4flex_frame_assemble_device(const void* src_base, const uint64_t* src_off, const uint32_t* in_len, const void* comp_base,
                                  const uint64_t* comp_off, const uint32_t* comp_len, uint32_t n, int block_checksums, void* seg,
                                  uint64_t* seg_off, void* scratch, void* hip_stream) {
    if (!seg_off || (n && (!src_base || !src_off || !in_len || !comp_base || !comp_off || !comp_len || !seg))) return -LZ4FLEX_E_INVALID_ARG;
    if (block_checksums && n && !scratch) return -LZ4FLEX_E_INVALID_ARG;
    uint8_t* sc = (uint8_t*)scratch;                                     // 16 bytes per block: u64 payload offset, u32 length, u32 XXH32
    hipError_t le = launch_frame_assemble((const uint8_t*)src_base, src_off, in_len, (const uint8_t*)comp_base, comp_off, comp_len, n,
                                          block_checksums, (uint8_t*)seg, seg_off, (uint64_t*)sc, (uint32_t*)(sc + 8ull * n),
                                          (uint32_t*)(sc + 12ull * n), (hipStream_t)hip_stream);
    return le == hipSuccess ? 0 : hip_fail(le, "frame assemble launch");
}

int lz4flex_copy_batch_device(const void* src_base, const uint64_t* src_off, const uint32_t* len, void* dst_base, const uint64_t* dst_off,
                              uint32_t n, void* hip_stream) {
    if (n && (!src_base || !src_off || !len || !dst_base || !dst_off)) return -LZ4FLEX_E_INVALID_ARG;
    hipError_t le = launch_copy_batch((const uint8_t*)src_base, src_off, len, (uint8_t*)dst_base, dst_off, n, (hipStream_t)hip_stream);
    return le == hipSuccess ? 0 : hip_fail(le, "copy batch launch");
}

int lz4flex_frame_walk_device(const void* frame, uint64_t frame_len, uint32_t header_len, int block_checksums, uint32_t block_size,
                              uint32_t max_blocks, uint64_t* payload_off, uint32_t* len_word, uint32_t* info, void* hip_stream) {
    if (!frame || !payload_off || !len_word || !info) return -LZ4FLEX_E_INVALID_ARG;
    hipError_t le = launch_frame_walk((const uint8_t*)frame, frame_len, header_len, block_checksums ? 4u : 0u, block_size, max_blocks,
                                      payload_off, len_word, info, (hipStream_t)hip_stream);
    return le == hipSuccess ? 0 : hip_fail(le, "frame walk launch");
}

// ---- CompressTable / compress_into_with_table, src/block/compress.rs:710-766 --------------------------------------
// The reference clears the table on every call: the handle only avoids re-allocating it and remembers its variant
// (Small = u16 entries + 4-byte hash, Large = u32 entries + 5-byte hash; upgraded, never downgraded).  Here the handle
// owns a context, i.e. the device workspace that is reused from call to call.
struct lz4flex_compress_table {
    lz4flex_ctx* ctx = nullptr;
    int large = 0;
};

lz4flex_compress_table* lz4flex_compress_table_new(int large) {
    lz4flex_compress_table* t = new (std::nothrow) lz4flex_compress_table();
    if (!t) return nullptr;
    t->large = large ? 1 : 0;
    if (lz4flex_ctx_create(&t->ctx, -1) != 0) { delete t; return nullptr; }
    return t;
}
void lz4flex_compress_table_free(lz4flex_compress_table* t) {
    if (!t) return;
    lz4flex_ctx_destroy(t->ctx);
    delete t;
}
int lz4flex_compress_table_is_large(const lz4flex_compress_table* t) { return t ? t->large : -LZ4FLEX_E_INVALID_ARG; }

int64_t lz4flex_compress_into_with_table(const uint8_t* in, size_t in_len, uint8_t* out, size_t out_cap, lz4flex_compress_table* t) {
    if (!t || in_len > 0xFFFFFFFFull) return -LZ4FLEX_E_INVALID_ARG;
    if (out_cap < lz4flex_get_maximum_output_size(in_len)) return -LZ4FLEX_E_OUTPUT_TOO_SMALL;   // compress.rs:338-340
    if (in_len >= 65535u) t->large = 1;                        // compress.rs:752-754: transparently upgraded, never downgraded
    lz4flex_ctx* dc = nullptr;
    int rc = default_ctx(&dc);
    if (rc) return rc;
    t->ctx->comp_mode = dc->comp_mode;                         // the thread's encoder choice (throughput / reference-exact / high)
    t->ctx->comp_depth = dc->comp_depth;
    t->ctx->comp_parse = dc->comp_parse;
    t->ctx->comp_high_dict = dc->comp_high_dict;
    t->ctx->comp_high_linked = dc->comp_high_linked;
    t->ctx->comp_variant = dc->comp_variant;
    const uint32_t len = (uint32_t)in_len, cap = (uint32_t)std::min<size_t>(out_cap, 0xFFFFFFFFull);
    // Large: HashTable4K, cleared, stream offset 0 == the frame encoder's first block (LZ4FLEX_BLOCK_FRAME_FIRST);
    // Small: what compress_into picks for inputs below 65 535 bytes
    const uint32_t flags = t->large ? LZ4FLEX_BLOCK_FRAME_FIRST : LZ4FLEX_BLOCK_DEFAULT;
    uint32_t olen = 0;
    int32_t st = 0;
    BatchCall b = batch_of(true, in ? in : &EMPTY, &OFF0, &len, 1, out, &OFF0, &cap, &olen, &st);
    b.flags = &flags;
    rc = run_host_batch(t->ctx, b);
    if (rc) return rc;
    if (st) return -(int64_t)st;
    return (int64_t)olen;
}

// compress_prepend_size_with_dict, src/block/compress.rs:692-694: LE u32 length, then compress_into_with_dict's block
int64_t lz4flex_compress_prepend_size_with_dict(const uint8_t* in, size_t in_len, uint8_t* out, size_t out_cap, const uint8_t* dict,
                                                size_t dict_len) {
    if (in_len > 0x7FFFFFFFull) return -LZ4FLEX_E_INVALID_ARG;
    if (out_cap < 4 || out_cap - 4 < lz4flex_get_maximum_output_size(in_len)) return -LZ4FLEX_E_OUTPUT_TOO_SMALL;
    const uint32_t n = (uint32_t)in_len;
    out[0] = (uint8_t)n; out[1] = (uint8_t)(n >> 8); out[2] = (uint8_t)(n >> 16); out[3] = (uint8_t)(n >> 24);
    // compress_into_vec_with_dict: dictionaries of <= 3 bytes are ignored (compress.rs:626-628)
    const int64_t r = dict_len <= 3 ? lz4flex_compress_into(in, in_len, out + 4, out_cap - 4)
                                    : lz4flex_compress_into_with_dict(in, in_len, out + 4, out_cap - 4, dict, dict_len);
    return r < 0 ? r : r + 4;
}

int64_t lz4flex_uncompressed_size(const uint8_t* in, size_t in_len) {
    if (in_len < 4) return -LZ4FLEX_E_EXPECTED_ANOTHER_BYTE;   // mod.rs:152
    return (int64_t)((uint32_t)in[0] | ((uint32_t)in[1] << 8) | ((uint32_t)in[2] << 16) | ((uint32_t)in[3] << 24));
}

int64_t lz4flex_decompress_size_prepended(const uint8_t* in, size_t in_len, uint8_t* out, size_t out_cap,
                                          lz4flex_err_detail* detail) {
    const int64_t sz = lz4flex_uncompressed_size(in, in_len);
    if (sz < 0) return sz;
    if ((uint64_t)sz > out_cap) return -LZ4FLEX_E_INVALID_ARG;   // the Vec variant allocates `sz`; here the caller must
    // decompress.rs:493-496 -> decompress(input, uncompressed_size): capacity is exactly the prefix
    return decompress_common(in + 4, in_len - 4, out, (size_t)sz, nullptr, 0, false, detail);
}

// decompress_size_prepended_with_dict, src/block/decompress.rs:521-527
int64_t lz4flex_decompress_size_prepended_with_dict(const uint8_t* in, size_t in_len, uint8_t* out, size_t out_cap, const uint8_t* dict,
                                                    size_t dict_len, lz4flex_err_detail* detail) {
    const int64_t sz = lz4flex_uncompressed_size(in, in_len);
    if (sz < 0) return sz;
    if ((uint64_t)sz > out_cap) return -LZ4FLEX_E_INVALID_ARG;   // the Vec variant allocates `sz`; here the caller must
    return decompress_common(in + 4, in_len - 4, out, (size_t)sz, dict, dict_len, true, detail);
}

}  // extern "C"
