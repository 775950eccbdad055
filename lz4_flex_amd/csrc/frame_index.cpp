// frame_index.cpp -- seekable frames: lz4flex_frame_index_create / lz4flex_frame_read_ranges (include/lz4flex_amd.h).
//
// What it replaces: FrameDecoder (src/frame/decompress.rs:189-342) read from the frame's first byte up to the bytes that are wanted --
// the reference has no random access, and neither had this library's frame layer: every entry decodes a frame from end to end.  An
// Independent frame is a sequence of blocks that do not need each other, so the block table -- where each block's payload lies and
// which content bytes it holds -- is all a reader needs to decode only the blocks a byte range touches:
//   create: the header on the host (lz4flex_frame_info_read), the BlockInfo walk on the device (launch_frame_walk), the decoded size of
//           every compressed block from the size scan (launch_size_scan, nothing is decoded), the content offsets from the packed
//           scan (launch_packed_scan, align 1).  The three tables stay in device memory the index owns, with a host copy beside them.
//   read:   the host locates every range in the host copy (frame_range.h: binary search, head detection, passes), one record per range
//           goes up, frame_range_plan_kernel turns the records into the items of two partial-decode batches and two copy batches from the
//           DEVICE tables, the existing launches run over them, frame_range_verdict_kernel folds the items' results into one verdict
//           per range, and m results come back.
// A block is decoded from ITS first byte (LZ4 has no other way in), up to the last byte that is wanted (lz4flex_decompress_batch_partial):
// straight into the caller's buffer when the range wants the block's start, else into scratch, from where the wanted bytes are copied
// (a "head": at most one per range).  Ranges that touch the same block decode it once each.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/lz4flex_amd.h"
#include "frame_cols.h"
#include "frame_plan.h"
#include "frame_range.h"
#include "frame_try.h"
#include "lz4_ctx.h"
#include "lz4_device.h"

struct lz4flex_frame_index {
    int device = 0;
    uint32_t blocks = 0;
    uint64_t content_size = 0, frame_bytes = 0;
    lz4flex_frame_info info{};
    uint32_t block_bytes = 0;                 // the frame's block size
    uint8_t* mem = nullptr;                   // device: [content_off (blocks + 1) | payload_off | len_word], nothing writes it after create
    const uint64_t* d_content = nullptr;
    const uint64_t* d_payload = nullptr;
    const uint32_t* d_word = nullptr;
    std::vector<uint64_t> content_off, payload_off;   // the host copy
    std::vector<uint32_t> len_word;
};

namespace {

using namespace lz4flex_dev;
using lz4flex_plan::block_size_bytes;
using lz4flex_range::RangeRec;

inline uint64_t up64(uint64_t v) { return (v + 63) / 64 * 64; }

// ---- create: f = the frame in device memory
int index_build(lz4flex_ctx* c, const uint8_t* f, uint64_t frame_len, const lz4flex_frame_info& fi, uint32_t hdr_len, lz4flex_frame_index* x,
                lz4flex_err_detail* detail, hipStream_t s) {
    const uint32_t bs = (uint32_t)block_size_bytes(fi.block_size), tail = fi.block_checksums ? 4u : 0u;
    // the table's size is not known before the walk: twice the full blocks the frame could hold, then -- the walk says "more" -- the most
    // a frame of that many bytes can hold at all (a block is at least its BlockInfo word)
    uint64_t max_blocks = frame_len / bs * 2 + 1024;
    const uint64_t most = frame_len / 4 + 1;
    void* w = nullptr;                                 // scratch slot 0 holds the columns; they have no host image
    IndexScratchCols a;
    uint32_t info[4] = {0, 0, 0, 0};
    for (;;) {
        max_blocks = std::min(max_blocks, most);
        if (max_blocks > 0x7FFFFFFFull) return -LZ4FLEX_E_UNSUPPORTED;
        const size_t mb = (size_t)max_blocks;
        ColumnPlan l(64);
        a = IndexScratchCols(l, mb, mb / PACKED_SCAN_TILE + 2);
        TRY_RC(ctx_scratch(c, 0, l.total() + 64, &w));
        TRY_HIP(launch_frame_walk(f, frame_len, hdr_len, tail, bs, (uint32_t)mb, ColumnPlan::view(w, a.pay), ColumnPlan::view(w, a.word),
                                  ColumnPlan::view(w, a.info), s));
        TRY_HIP(hipMemcpyAsync(info, ColumnPlan::view(w, a.info), 16, hipMemcpyDeviceToHost, s));
        TRY_HIP(hipStreamSynchronize(s));
        if (info[1] != 3u || max_blocks >= most) break;
        max_blocks = most;
    }
    uint32_t n = info[0], walk_st = info[1];
    uint64_t end = (uint64_t)info[2] | ((uint64_t)info[3] << 32);
    uint64_t *d_pay = ColumnPlan::view(w, a.pay), *d_size = ColumnPlan::view(w, a.size), *d_content = ColumnPlan::view(w, a.content);
    uint32_t *d_word = ColumnPlan::view(w, a.word), *d_scan_len = ColumnPlan::view(w, a.scan_len), *d_bad = ColumnPlan::view(w, a.bad);
    int32_t* d_scan_st = ColumnPlan::view(w, a.scan_st);
    // ---- decoded sizes and their exclusive sums
    TRY_HIP(launch_frame_index_prep(d_word, n, d_scan_len, d_bad, s));
    if (n) TRY_HIP(launch_size_scan(f, d_pay, d_scan_len, nullptr, n, d_size, d_scan_st, c->size_serial, s));
    TRY_HIP(launch_frame_index_sizes(d_word, d_scan_st, n, bs, d_size, d_bad, s));
    TRY_HIP(launch_packed_scan(d_size, n, 1u, ~0ull, 0u, ColumnPlan::view(w, a.tiles), d_content, nullptr, nullptr, nullptr, s));
    uint32_t firsts[2] = {0, 0};
    uint64_t total = 0;
    TRY_HIP(hipMemcpyAsync(firsts, d_bad, 8, hipMemcpyDeviceToHost, s));
    TRY_HIP(hipMemcpyAsync(&total, d_content + n, 8, hipMemcpyDeviceToHost, s));
    TRY_HIP(hipStreamSynchronize(s));
    const uint32_t first_bad = firsts[0], first_empty = firsts[1];
    // ---- the earliest defect in stream order (frame/decompress.rs:231-332): a block that does not decode, in front of where the walk stopped
    if (first_bad < n && first_bad < first_empty) {
        // its error is the decoder's own: once through the ordinary batch path, the sink a block size as FrameDecoder's is
        struct One { uint64_t out_off; uint64_t det[2]; uint32_t cap, olen; int32_t st; } one{0, {0, 0}, bs, 0, 0};
        uint8_t* d_one = ColumnPlan::view(w, a.one);
        void* sink = nullptr;
        TRY_RC(ctx_scratch(c, 1, (size_t)bs + 64, &sink));
        TRY_HIP(hipMemcpyAsync(d_one, &one, sizeof one, hipMemcpyHostToDevice, s));
        TRY_RC(lz4flex_decompress_batch(c, f, d_pay + first_bad, d_scan_len + first_bad, 1, sink, (const uint64_t*)(d_one + offsetof(One, out_off)),
                                        (const uint32_t*)(d_one + offsetof(One, cap)), (uint32_t*)(d_one + offsetof(One, olen)),
                                        (int32_t*)(d_one + offsetof(One, st)), (uint64_t*)(d_one + offsetof(One, det)),
                                        LZ4FLEX_MEM_DEVICE | (bs > 131072u ? LZ4FLEX_MEM_BIG_BLOCKS : 0), s));
        TRY_HIP(hipMemcpyAsync(&one, d_one, sizeof one, hipMemcpyDeviceToHost, s));
        TRY_HIP(hipStreamSynchronize(s));
        if (detail) { detail->inner = one.st; detail->expected = one.det[0]; detail->actual = one.det[1]; }
        return -LZ4FLEX_FE_DECOMPRESSION;
    }
    bool open_end = false;
    if (first_empty < n) {
        // A block of no bytes ends the reader's read_to_end with the content in front of it (frame/decompress.rs:344-349,392-407: no
        // EndMark is reached, so neither the content size nor anything behind that block is looked at): the index is of the blocks in
        // front of it and the frame ends behind it.
        uint64_t pay = 0;
        uint32_t word = 0;
        TRY_HIP(hipMemcpyAsync(&total, d_content + first_empty, 8, hipMemcpyDeviceToHost, s));
        TRY_HIP(hipMemcpyAsync(&pay, d_pay + first_empty, 8, hipMemcpyDeviceToHost, s));
        TRY_HIP(hipMemcpyAsync(&word, d_word + first_empty, 4, hipMemcpyDeviceToHost, s));
        TRY_HIP(hipStreamSynchronize(s));
        n = first_empty; walk_st = 0u; open_end = true;
        end = pay + (word & 0x7FFFFFFFu) + tail;
    }
    if (walk_st == 1u) return -LZ4FLEX_FE_IO;
    if (walk_st == 2u) return -LZ4FLEX_FE_BLOCK_TOO_BIG;
    if (walk_st != 0u) return -LZ4FLEX_E_UNSUPPORTED;
    if (!open_end && fi.has_content_size && fi.content_size != total) {             // :313-320
        if (detail) { detail->expected = fi.content_size; detail->actual = total; }
        return -LZ4FLEX_FE_CONTENT_LENGTH;
    }
    const uint64_t frame_bytes = end + (fi.content_checksum && !open_end ? 4u : 0u);
    if (frame_bytes > frame_len) return -LZ4FLEX_FE_IO;                             // (the content checksum's bytes: :321-326)
    // ---- the index's own copy
    ColumnPlan o(64);
    const IndexTableCols t(o, n);
    TRY_HIP(hipMalloc((void**)&x->mem, o.total() + 64));
    uint64_t *x_content = ColumnPlan::view(x->mem, t.content), *x_pay = ColumnPlan::view(x->mem, t.pay);
    uint32_t* x_word = ColumnPlan::view(x->mem, t.word);
    x->content_off.resize((size_t)n + 1); x->payload_off.resize(n); x->len_word.resize(n);
    TRY_HIP(hipMemcpyAsync(x_content, d_content, 8ull * (n + 1), hipMemcpyDeviceToDevice, s));
    TRY_HIP(hipMemcpyAsync(x->content_off.data(), d_content, 8ull * (n + 1), hipMemcpyDeviceToHost, s));
    if (n) {
        TRY_HIP(hipMemcpyAsync(x_pay, d_pay, 8ull * n, hipMemcpyDeviceToDevice, s));
        TRY_HIP(hipMemcpyAsync(x_word, d_word, 4ull * n, hipMemcpyDeviceToDevice, s));
        TRY_HIP(hipMemcpyAsync(x->payload_off.data(), d_pay, 8ull * n, hipMemcpyDeviceToHost, s));
        TRY_HIP(hipMemcpyAsync(x->len_word.data(), d_word, 4ull * n, hipMemcpyDeviceToHost, s));
    }
    TRY_HIP(hipStreamSynchronize(s));
    x->d_content = x_content; x->d_payload = x_pay; x->d_word = x_word;
    x->device = c->device; x->blocks = n; x->content_size = total; x->frame_bytes = frame_bytes; x->info = fi; x->block_bytes = bs;
    return 0;
}

// ---- one pass of ranges: in / out are device memory, the records' out_off / shift / head_off / slot are set
struct PassOut { int32_t* status; uint64_t* out_len; lz4flex_err_detail* detail; };

int run_pass(lz4flex_ctx* c, const lz4flex_frame_index* x, const uint8_t* in, uint8_t* out, const RangeRec* recs, uint32_t R, uint32_t T,
             uint64_t head_total, const PassOut& res, hipStream_t s) {
    Desc D;
    const RangePassCols a(D, R, T);
    D.fill(a.rec, recs);
    void* p = nullptr;
    TRY_RC(ctx_scratch(c, 0, D.total() + 64, &p));
    TRY_HIP(D.upload(p, D.up_bytes, s));               // (the records: everything behind them is written by the device)
    void* heads = nullptr;
    if (head_total) TRY_RC(ctx_scratch(c, 1, (size_t)head_total + 64, &heads));
    FrameRangePlan pl{};
    pl.rec = D.dev(a.rec); pl.content_off = x->d_content; pl.payload_off = x->d_payload; pl.len_word = x->d_word;
    pl.n_ranges = R; pl.n_slots = T;
    pl.a_in = D.dev(a.a_in); pl.a_out = D.dev(a.a_out); pl.a_len = D.dev(a.a_len); pl.a_tgt = D.dev(a.a_tgt);
    pl.b_in = D.dev(a.b_in); pl.b_out = D.dev(a.b_out); pl.b_len = D.dev(a.b_len); pl.b_tgt = D.dev(a.b_tgt);
    pl.c_src = D.dev(a.c_src); pl.c_dst = D.dev(a.c_dst); pl.c_len = D.dev(a.c_len);
    pl.d_src = D.dev(a.d_src); pl.d_dst = D.dev(a.d_dst); pl.d_len = D.dev(a.d_len);
    TRY_HIP(launch_frame_range_plan(pl, s));
    const bool sums = x->info.block_checksums && c->range_checksums && T;
    if (sums) {                                        // frame/decompress.rs:255-261,275-278: the whole payload, before anything is decoded
        TRY_HIP(launch_xxh32_batch(in, pl.a_in, pl.a_len, T, 0u, D.dev(a.k_sum), s));
        TRY_HIP(launch_frame_sums_check(in, pl.a_in, pl.a_len, D.dev(a.k_sum), T, D.dev(a.k_bad), s));
    }
    const int big = x->block_bytes > 131072u ? LZ4FLEX_MEM_BIG_BLOCKS : 0;
    if (T)
        TRY_RC(lz4flex_decompress_batch_partial(c, in, pl.a_in, pl.a_len, T, out, pl.a_out, pl.a_tgt, D.dev(a.a_olen), D.dev(a.a_st),
                                                LZ4FLEX_MEM_DEVICE | big, s));
    if (head_total)
        TRY_RC(lz4flex_decompress_batch_partial(c, in, pl.b_in, pl.b_len, R, heads, pl.b_out, pl.b_tgt, D.dev(a.b_olen), D.dev(a.b_st),
                                                LZ4FLEX_MEM_DEVICE | big, s));
    TRY_HIP(launch_copy_batch(in, pl.c_src, pl.c_len, out, pl.c_dst, T, s));                                   // stored blocks (:262-271)
    if (head_total) TRY_HIP(launch_copy_batch((const uint8_t*)heads, pl.d_src, pl.d_len, out, pl.d_dst, R, s));
    FrameRangeVerdict v{};
    v.rec = pl.rec; v.len_word = x->d_word; v.n_ranges = R; v.bad = sums ? D.dev(a.k_bad) : nullptr;
    v.a_st = D.dev(a.a_st); v.b_st = D.dev(a.b_st); v.a_tgt = pl.a_tgt; v.a_olen = D.dev(a.a_olen);
    v.b_tgt = pl.b_tgt; v.b_olen = D.dev(a.b_olen);
    v.status = D.dev(a.v_st); v.inner = D.dev(a.v_inner); v.out_len = D.dev(a.v_len);
    v.expected = D.dev(a.v_exp); v.actual = D.dev(a.v_act);
    TRY_HIP(launch_frame_range_verdict(v, s));
    TRY_HIP(D.fetch_columns(a.v_st, s));               // the five verdict columns, one copy
    TRY_HIP(hipStreamSynchronize(s));
    for (uint32_t r = 0; r < R; r++) {
        res.status[r] = D.host(a.v_st)[r];
        res.out_len[r] = D.host(a.v_len)[r];
        if (res.detail) {
            memset(&res.detail[r], 0, sizeof res.detail[r]);
            res.detail[r].inner = D.host(a.v_inner)[r];
            res.detail[r].expected = D.host(a.v_exp)[r];
            res.detail[r].actual = D.host(a.v_act)[r];
        }
    }
    return 0;
}

int read_ranges(lz4flex_ctx* c, const lz4flex_frame_index* x, const uint8_t* frame, const uint64_t* range_off, const uint64_t* range_len, uint32_t m,
                uint8_t* out_base, const uint64_t* out_off, uint64_t* out_len, int32_t* status, lz4flex_err_detail* detail, bool host, hipStream_t s) {
    const uint32_t n = x->blocks, tail = x->info.block_checksums ? 4u : 0u;
    std::vector<RangeRec> recs(m);
    std::vector<uint64_t> cost(m), span_lo(host ? m : 0), span_len(host ? m : 0);
    for (uint32_t r = 0; r < m; r++) {
        RangeRec& q = recs[r];
        memset(&q, 0, sizeof q);
        lz4flex_range::locate(x->content_off.data(), x->len_word.data(), n, range_off[r], range_len[r], &q);
        q.out_off = out_off[r];
        cost[r] = lz4flex_range::head_slot_bytes(q);
        if (host && q.nb) {
            // the frame span a range needs: from its first block's BlockInfo word to the end of its last block, checksum word included
            const uint32_t b1 = q.b0 + q.nb - 1;
            span_lo[r] = x->payload_off[q.b0] - 4;
            span_len[r] = x->payload_off[b1] + (x->len_word[b1] & 0x7FFFFFFFu) + tail - span_lo[r];
            cost[r] += up64(span_len[r]) + up64(q.len);
        }
    }
    const uint64_t pass_bytes = (uint64_t)std::max(c->range_pass_bytes, 1);
    for (uint32_t first = 0; first < m;) {
        uint64_t slots = 0, head_total = 0;
        const uint32_t cnt = lz4flex_range::cut_pass(recs.data(), cost.data(), first, m, pass_bytes, &slots, &head_total);
        if (slots > 0x7FFFFFFFull) return -LZ4FLEX_E_UNSUPPORTED;
        const PassOut res{status + first, out_len + first, detail ? detail + first : nullptr};
        if (!host) {
            TRY_RC(run_pass(c, x, frame, out_base, recs.data() + first, cnt, (uint32_t)slots, head_total, res, s));
            first += cnt;
            continue;
        }
        // MEM_HOST: the spans and the outputs of the pass are staged back to back (scratch slots 2 and 3)
        uint64_t in_bytes = 0, out_bytes = 0;
        for (uint32_t r = first; r < first + cnt; r++) {
            recs[r].shift = (int64_t)in_bytes - (int64_t)span_lo[r];
            recs[r].out_off = out_bytes;
            in_bytes += up64(span_len[r]); out_bytes += up64(recs[r].len);
        }
        void *d_in = nullptr, *d_out = nullptr;
        TRY_RC(ctx_scratch(c, 2, (size_t)in_bytes + 64, &d_in));
        TRY_RC(ctx_scratch(c, 3, (size_t)out_bytes + 64, &d_out));
        for (uint32_t r = first; r < first + cnt; r++)
            if (span_len[r])
                TRY_HIP(hipMemcpyAsync((uint8_t*)d_in + (span_lo[r] + recs[r].shift), frame + span_lo[r], (size_t)span_len[r], hipMemcpyHostToDevice, s));
        TRY_RC(run_pass(c, x, (const uint8_t*)d_in, (uint8_t*)d_out, recs.data() + first, cnt, (uint32_t)slots, head_total, res, s));
        for (uint32_t r = first; r < first + cnt; r++)
            if (status[r] == 0 && out_len[r])
                TRY_HIP(hipMemcpyAsync(out_base + out_off[r], (const uint8_t*)d_out + recs[r].out_off, (size_t)out_len[r], hipMemcpyDeviceToHost, s));
        TRY_HIP(hipStreamSynchronize(s));
        first += cnt;
    }
    return 0;
}

}  // namespace

extern "C" {

int lz4flex_frame_index_create(lz4flex_ctx* ctx, const void* frame, uint64_t frame_len, int mem_kind, lz4flex_frame_index** out,
                               lz4flex_err_detail* detail) {
    if (out) *out = nullptr;
    if (detail) memset(detail, 0, sizeof *detail);
    if (!out || !frame || (mem_kind != LZ4FLEX_MEM_HOST && mem_kind != LZ4FLEX_MEM_DEVICE)) return -LZ4FLEX_E_INVALID_ARG;
    TRY_RC(ctx_resolve(&ctx));
    lz4flex_frame_index* x = nullptr;
    int rc = 0;
    try {
        DeviceGuard guard(ctx->device);
        TRY_HIP(guard.err);
        hipStream_t s = ctx->stream;
        // ---- the header, on the host (FrameInfo::read, frame/header.rs:277-373)
        uint8_t head[32] = {0};
        const size_t hn = (size_t)std::min<uint64_t>(frame_len, sizeof head);
        if (mem_kind == LZ4FLEX_MEM_HOST) memcpy(head, frame, hn);
        else if (hn) { TRY_HIP(hipMemcpyAsync(head, frame, hn, hipMemcpyDeviceToHost, s)); TRY_HIP(hipStreamSynchronize(s)); }
        lz4flex_frame_info fi;
        const int64_t hl = lz4flex_frame_info_read(head, hn, &fi, detail);
        if (hl < 0) return (int)hl;
        // a Linked block needs the 64 KiB in front of it, and so on back to the frame's start: nothing to seek in; legacy frames have no BlockInfo flags
        if (fi.legacy_frame || fi.block_mode == 1 || block_size_bytes(fi.block_size) == 0) return -LZ4FLEX_E_UNSUPPORTED;
        const uint8_t* f = (const uint8_t*)frame;
        if (mem_kind == LZ4FLEX_MEM_HOST) {              // staged once, as lz4flex_frame_decompress_many stages its input
            void* d = nullptr;
            TRY_RC(ctx_scratch(ctx, 2, (size_t)frame_len + 64, &d));
            TRY_HIP(hipMemcpyAsync(d, frame, (size_t)frame_len, hipMemcpyHostToDevice, s));
            f = (const uint8_t*)d;
        }
        x = new lz4flex_frame_index();
        rc = index_build(ctx, f, frame_len, fi, (uint32_t)hl, x, detail, s);
    } catch (...) { rc = -LZ4FLEX_E_NOMEM; }
    if (rc) { lz4flex_frame_index_free(x); return rc; }
    *out = x;
    return 0;
}

void lz4flex_frame_index_free(lz4flex_frame_index* x) {
    if (!x) return;
    if (x->mem) {
        DeviceGuard guard(x->device);
        (void)hipFree(x->mem);
    }
    delete x;
}

uint32_t lz4flex_frame_index_blocks(const lz4flex_frame_index* x) { return x ? x->blocks : 0u; }
uint64_t lz4flex_frame_index_content_size(const lz4flex_frame_index* x) { return x ? x->content_size : 0ull; }
uint64_t lz4flex_frame_index_frame_bytes(const lz4flex_frame_index* x) { return x ? x->frame_bytes : 0ull; }
void lz4flex_frame_index_info(const lz4flex_frame_index* x, lz4flex_frame_info* out) {
    if (x && out) *out = x->info;
}
int lz4flex_frame_index_table(const lz4flex_frame_index* x, uint64_t* content_off, uint64_t* payload_off, uint32_t* len_word) {
    if (!x) return -LZ4FLEX_E_INVALID_ARG;
    if (content_off) memcpy(content_off, x->content_off.data(), 8ull * (x->blocks + 1ull));
    if (payload_off && x->blocks) memcpy(payload_off, x->payload_off.data(), 8ull * x->blocks);
    if (len_word && x->blocks) memcpy(len_word, x->len_word.data(), 4ull * x->blocks);
    return 0;
}

int lz4flex_frame_read_ranges(lz4flex_ctx* ctx, const lz4flex_frame_index* x, const void* frame, const uint64_t* range_off, const uint64_t* range_len,
                              uint32_t m, void* out_base, const uint64_t* out_off, uint64_t* out_len, int32_t* status, lz4flex_err_detail* detail,
                              int mem_kind, void* hip_stream) {
    if (!x || (mem_kind != LZ4FLEX_MEM_HOST && mem_kind != LZ4FLEX_MEM_DEVICE)) return -LZ4FLEX_E_INVALID_ARG;
    if (m == 0) return 0;
    if (!frame || !range_off || !range_len || !out_base || !out_off || !out_len || !status) return -LZ4FLEX_E_INVALID_ARG;
    TRY_RC(ctx_resolve(&ctx));
    if (ctx->device != x->device) return -LZ4FLEX_E_INVALID_ARG;
    try {
        DeviceGuard guard(ctx->device);
        TRY_HIP(guard.err);
        const bool host = mem_kind == LZ4FLEX_MEM_HOST;
        return read_ranges(ctx, x, (const uint8_t*)frame, range_off, range_len, m, (uint8_t*)out_base, out_off, out_len, status, detail, host,
                           host ? ctx->stream : (hipStream_t)hip_stream);
    } catch (...) { return -LZ4FLEX_E_NOMEM; }
}

}  // extern "C"
