// frame_many.cpp -- N frames at once: lz4flex_frame_compress_many / lz4flex_frame_decompress_many (include/lz4flex_amd.h).
//
// What it replaces: N FrameEncoders / FrameDecoders (src/frame/compress.rs:261-371, src/frame/decompress.rs:189-342), one per
// stream, each running its own sequence of block codec calls -- the reference's answer to many streams is one thread per stream.
// A Linked frame is ONE dependency chain (every block's matches reach into the block before it, decompress.rs:195-222): a single
// stream gives a GPU nothing to do side by side, N streams give it N chains.  Here the blocks of ALL streams form one batch:
//   encode: one launch of the block encoder over every block of every stream (throughput encoder: a Linked block's history is input,
//           LZ4FLEX_BLOCK_HISTORY; reference-exact mode: lz4flex_compress_chains, N chains side by side), then one thread per stream
//           lays the frame out (header, BlockInfo words, EndMark, content checksum) and one workgroup per block moves its payload;
//   decode: the headers come to the host (32 bytes per frame), one thread per frame walks its BlockInfo words, the host turns the
//           tables into ONE batch -- Independent frames: plain blocks; Linked frames: a chained batch of N chains ordered level by
//           level (every stream's block k before any stream's block k + 1, lz4flex_decompress_ext::chain_prev), so that all chains
//           advance together and a block waits for its own predecessor only.
// A decoded size is not in the frame: every block but a frame's last is taken to fill the block size.  Whatever does not fit that
// picture -- a frame that does not parse, a flush() boundary inside a frame, an empty block, a block or content
// checksum that does not match, a decode error, a buffer too small -- is decoded AGAIN by lz4flex_frame_decompress (the streaming
// decoder over this library's kernels), which has the reference's order of checks and names the error: the fast path never reports
// an error of its own.  The same on the encode side for streams of 2 GiB and more (lz4flex_frame_compress).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/lz4flex_amd.h"
#include "frame_cols.h"
#include "frame_plan.h"
#include "frame_try.h"
#include "lz4_batch_entry.h"
#include "lz4_ctx.h"
#include "lz4_device.h"

namespace {

using namespace lz4flex_dev;
using namespace lz4flex_plan;   // block sizes, FAST_HISTORY, STREAM_MAX (the streams the batch path takes), TableOffset, LinkedWindow

// ("decompress_level_chains", default 1 024: from this many Linked streams in one call on their blocks are decoded a level per launch -- the groups loop)
constexpr uint64_t MAX_SLOTS = 1ull << 26;               // block-table entries per decompress_many call (12 bytes each on the host and on the device)

// descriptor columns (Desc, lz4_ctx.h; their names: frame_cols.h): the device copy is scratch slot 0, the WHOLE image goes up, the
// zeros of the result columns included
int upload(lz4flex_ctx* c, Desc& D, hipStream_t s) {
    void* p = nullptr;
    TRY_RC(ctx_scratch(c, 0, D.total() + 64, &p));
    TRY_HIP(D.upload(p, D.total(), s));
    return 0;
}

// ---- the streams the batch path leaves out: FrameEncoder / FrameDecoder over flat buffers, one stream at a time
int compress_one(const uint8_t* d_in, uint64_t len, const lz4flex_frame_info* info, uint8_t* d_out, uint64_t cap, uint64_t* out_len,
                 int32_t* status, hipStream_t s) {
    std::vector<uint8_t> in((size_t)len), out((size_t)std::min<uint64_t>(cap, lz4flex_frame_compress_bound((size_t)len, info)));
    if (len) TRY_HIP(hipMemcpyAsync(in.data(), d_in, (size_t)len, hipMemcpyDeviceToHost, s));
    TRY_HIP(hipStreamSynchronize(s));
    const int64_t rc = lz4flex_frame_compress(in.data(), in.size(), info, out.data(), out.size(), nullptr);
    *status = rc < 0 ? (int32_t)rc : 0;
    *out_len = rc < 0 ? 0 : (uint64_t)rc;
    if (rc > 0) { TRY_HIP(hipMemcpyAsync(d_out, out.data(), (size_t)rc, hipMemcpyHostToDevice, s)); TRY_HIP(hipStreamSynchronize(s)); }
    return 0;
}
int decompress_one(const uint8_t* d_in, uint64_t len, uint8_t* d_out, uint64_t cap, uint64_t* out_len, int32_t* status,
                   lz4flex_err_detail* detail, hipStream_t s) {
    // (an "unbounded" out_cap must not become a host allocation of that size: LZ4 expands at most 255 x)
    const uint64_t most = len > (1ull << 40) ? cap : std::min<uint64_t>(cap, 255ull * len + 64u);
    std::vector<uint8_t> in((size_t)len), out((size_t)most);
    if (len) TRY_HIP(hipMemcpyAsync(in.data(), d_in, (size_t)len, hipMemcpyDeviceToHost, s));
    TRY_HIP(hipStreamSynchronize(s));
    static uint8_t none = 0;
    const int64_t rc = lz4flex_frame_decompress(len ? in.data() : &none, in.size(), cap ? out.data() : &none, out.size(), nullptr, detail);
    *status = rc < 0 ? (int32_t)rc : 0;
    *out_len = rc < 0 ? 0 : (uint64_t)rc;
    if (rc > 0) { TRY_HIP(hipMemcpyAsync(d_out, out.data(), (size_t)rc, hipMemcpyHostToDevice, s)); TRY_HIP(hipStreamSynchronize(s)); }
    return 0;
}

// =============================================================================================================== encode
int compress_many_device(lz4flex_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n,
                         const lz4flex_frame_info* info, uint8_t* out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len,
                         int32_t* status, hipStream_t s) {
    const bool linked = info->block_mode == 1, exact = c->comp_mode == 1;
    const bool bsum = info->block_checksums != 0, csum = info->content_checksum != 0;
    // ---- which streams go through the batch, and their blocks
    std::vector<uint32_t> fast;                        // stream indices
    std::vector<uint32_t> slow;
    std::vector<int> code(n, 0);
    uint64_t nb64 = 0;
    for (uint32_t i = 0; i < n; i++) {
        code[i] = info->block_size ? info->block_size : block_size_from_buf_length(in_len[i]);
        const size_t mbs = block_size_bytes(code[i]);
        if (mbs == 0 || code[i] == 8) return -LZ4FLEX_E_INVALID_ARG;                   // (Max8MB is legacy-decode only, frame/header.rs:287)
        if (in_len[i] > STREAM_MAX) { slow.push_back(i); continue; }
        fast.push_back(i);
        nb64 += (in_len[i] + mbs - 1) / mbs;
    }
    if (nb64 > 0x7FFFFFFFull) return -LZ4FLEX_E_INVALID_ARG;
    const uint32_t nb = (uint32_t)nb64, nf = (uint32_t)fast.size();
    Desc D;
    const ManyEncodeCols<ManyStream> a(D, nf, nb, exact && linked);
    uint64_t comp_bytes = 0;
    bool big = false;
    {
        ManyStream* ms = D.host(a.ms);
        uint64_t *soff = D.host(a.soff), *b_in = D.host(a.in_off), *b_co = D.host(a.comp_off);
        uint32_t *slen = D.host(a.slen), *b_len = D.host(a.in_len), *b_fl = D.host(a.flags), *b_cap = D.host(a.comp_cap);
        lz4flex_chain_block* cb = (exact && linked) ? D.host(a.cb) : nullptr;
        uint32_t b = 0;
        for (uint32_t f = 0; f < nf; f++) {
            const uint32_t i = fast[f];
            const size_t mbs = block_size_bytes(code[i]);
            big |= mbs > 65536;
            const uint32_t cnt = (uint32_t)((in_len[i] + mbs - 1) / mbs);
            ManyStream& m = ms[f];
            m.out_off = out_off[i]; m.out_cap = out_cap[i]; m.first = b; m.count = cnt;
            m.flags = (bsum ? 1u : 0u) | (csum ? 2u : 0u);
            lz4flex_frame_info fi = *info;
            fi.block_size = code[i];
            if (fi.has_content_size) fi.content_size = in_len[i];                      // every frame carries ITS stream's length
            const int64_t hl = lz4flex_frame_info_write(&fi, m.hdr, sizeof m.hdr);
            if (hl < 0) return (int)hl;
            m.hdr_len = (uint32_t)hl;
            soff[f] = in_off[i]; slen[f] = (uint32_t)in_len[i];
            if (cb) { D.host(a.first)[f] = b; D.host(a.count)[f] = cnt; }
            // table mode (Independent) / window (Linked) of the reference's encoder, block after block: frame_plan.h.  No stream here
            // is longer than STREAM_MAX, so neither ever repositions: FRAME_FIRST is block 0 alone, every chain block's repos is 0
            TableOffset tbl;
            LinkedWindow win;
            for (uint32_t k = 0; k < cnt; k++, b++) {
                const uint64_t at = (uint64_t)k * mbs;
                const uint32_t len = (uint32_t)std::min<uint64_t>(mbs, in_len[i] - at);
                b_in[b] = in_off[i] + at; b_len[b] = len;
                b_cap[b] = (uint32_t)((lz4flex_get_maximum_output_size(len) + 63) / 64 * 64);
                b_co[b] = comp_bytes; comp_bytes += b_cap[b];
                if (!exact) b_fl[b] = (linked && k > 0) ? LZ4FLEX_BLOCK_HISTORY(std::min<uint64_t>(at, FAST_HISTORY)) : 0u;
                else b_fl[b] = tbl.next(mbs, len);                                         // (read by the Independent path only)
                if (cb) {
                    lz4flex_chain_block& q = cb[b];
                    q = win.next(mbs, len);                                                // (stream positions; the stream starts at in_off[i])
                    q.in_off += in_off[i];
                    if (q.dict_len) q.dict_off += in_off[i];
                }
            }
        }
    }
    TRY_RC(upload(c, D, s));
    void* comp = nullptr;
    TRY_RC(ctx_scratch(c, 1, (size_t)comp_bytes + 64, &comp));
    if (nb) {
        if (exact && linked)
            TRY_RC(lz4flex_compress_chains(c, in, D.dev(a.cb), nb, D.dev(a.first), D.dev(a.count), nf, comp, D.dev(a.comp_off), D.dev(a.comp_cap),
                                           D.dev(a.comp_len), D.dev(a.comp_st), nullptr, LZ4FLEX_MEM_DEVICE, s));
        else
            // (one launch over all blocks of all streams; `linked`: what compress_mode high does with a Linked frame's blocks is
            // encode_route's rule, lz4_route.h)
            TRY_RC(compress_batch_entry(c, in, D.dev(a.in_off), D.dev(a.in_len), D.dev(a.flags), nb, comp, D.dev(a.comp_off), D.dev(a.comp_cap),
                                        D.dev(a.comp_len), D.dev(a.comp_st), LZ4FLEX_MEM_DEVICE | (big ? LZ4FLEX_MEM_BIG_BLOCKS : 0), s, linked));
    }
    if (csum && nf) TRY_RC(lz4flex_xxh32_batch_device(in, D.dev(a.soff), D.dev(a.slen), nf, 0, D.dev(a.csum), s));   // frame/compress.rs:319-321
    TRY_HIP(launch_frame_many_assemble(D.dev(a.ms), nf, in, D.dev(a.in_off), D.dev(a.in_len), (const uint8_t*)comp, D.dev(a.comp_off), D.dev(a.comp_len),
                                       D.dev(a.comp_st), nb, bsum ? 1 : 0, D.dev(a.csum), out, D.dev(a.dst_off), D.dev(a.pay_off), D.dev(a.pay_len),
                                       D.dev(a.sums), D.dev(a.flen), D.dev(a.verdict), s));
    TRY_HIP(D.fetch(a.flen, nf, s));
    TRY_HIP(D.fetch(a.verdict, nf, s));
    TRY_HIP(hipStreamSynchronize(s));
    for (uint32_t f = 0; f < nf; f++) {
        const uint32_t i = fast[f];
        const int32_t v = D.host(a.verdict)[f];
        status[i] = v == 0 ? 0 : (v == 1 ? -LZ4FLEX_FE_COMPRESSION : -LZ4FLEX_FE_OUTPUT_FULL);
        out_len[i] = v == 0 ? D.host(a.flen)[f] : 0;
    }
    for (uint32_t i : slow) {
        lz4flex_frame_info fi = *info;
        if (fi.has_content_size) fi.content_size = in_len[i];
        TRY_RC(compress_one(in + in_off[i], in_len[i], &fi, out + out_off[i], out_cap[i], &out_len[i], &status[i], s));
    }
    return 0;
}

// =============================================================================================================== decode
struct Entry {            // one compressed block of the batch
    uint32_t stream, k;   // its frame; its index among the frame's blocks
    uint64_t in_off, out_off;
    uint32_t in_len, cap, pos;
};

struct Group { size_t lo, hi; };   // the chained entries of one chained call: whole streams, at most CHAIN_MAX_BLOCKS blocks, ordered by (block index, stream)

// One call over device memory: its arguments, and what each of its four phases leaves for the next.  A phase ends where the stream is
// waited for; each runs once, in the order below.
struct ManyArgs {
    lz4flex_ctx* c;
    const uint8_t* in;
    const uint64_t *in_off, *in_len;
    uint32_t n;
    uint8_t* out;
    const uint64_t *out_off, *out_cap;
    hipStream_t s;
};
struct ManyDecode : ManyArgs {
    std::vector<uint8_t> again;                        // 1: the stream goes through lz4flex_frame_decompress
    std::vector<lz4flex_frame_info> fi;
    std::vector<uint8_t> heads;                        // 1 -> 2: the first 32 bytes of every frame
    Desc W;                                            // 2 -> 3, 4: the frames and their block tables
    ManyWalkCols<ManyFrame> wc;
    std::vector<Entry> plain, chained;                 // 3 -> 4: the batch, its image, and what the verdicts need of the stored blocks
    std::vector<Group> groups;
    std::vector<uint32_t> p_stream;                    // the stream of every block checksum
    std::vector<uint64_t> raw_bytes;                   // bytes of a stream's stored blocks
    uint32_t np = 0, nc = 0, nr = 0, nk = 0, ne = 0;
    Desc B;
    ManyBatchCols bc;
    explicit ManyDecode(const ManyArgs& a) : ManyArgs(a), again(n, 0), fi(n), heads(32ull * n), wc(W, n), raw_bytes(n, 0) {}
    int read_heads();
    int walk_tables();
    void build_batch();
    int run_batch();
    int finish(uint64_t* out_len, int32_t* status, lz4flex_err_detail* detail);
};

// ---- 1. headers
int ManyDecode::read_heads() {
    Desc H;
    const ManyHeadCols h(H, n);
    H.fill(h.off, in_off);
    H.fill(h.len, in_len);
    TRY_RC(upload(c, H, s));
    TRY_HIP(launch_frame_many_heads(in, H.dev(h.off), H.dev(h.len), n, H.dev(h.heads), s));
    TRY_HIP(hipMemcpyAsync(heads.data(), H.dev(h.heads), 32ull * n, hipMemcpyDeviceToHost, s));
    TRY_HIP(hipStreamSynchronize(s));
    return 0;
}

// ---- 2. the block tables
int ManyDecode::walk_tables() {
    uint64_t slots = 0;
    for (uint32_t i = 0; i < n; i++) {
        ManyFrame& m = W.host(wc.fr)[i];
        m.off = in_off[i]; m.len = in_len[i]; m.skip = 1;
        const int64_t hl = lz4flex_frame_info_read(heads.data() + 32ull * i, (size_t)std::min<uint64_t>(32, in_len[i]), &fi[i], nullptr);
        const size_t bs = hl < 0 ? 0 : block_size_bytes(fi[i].block_size);
        // (a header that does not parse, a legacy frame, an output a chained batch cannot address: the streaming decoder's business)
        if (hl < 0 || fi[i].legacy_frame || bs == 0 || (fi[i].block_mode == 1 && out_cap[i] > 0xFFFFFFFFull - 2 * bs)) { again[i] = 1; continue; }
        const uint64_t cap_blocks = out_cap[i] / bs + 2;
        if (slots + cap_blocks > MAX_SLOTS) { again[i] = 1; continue; }             // (a table of that size is not worth building: out_cap far beyond the data)
        m.hdr_len = (uint32_t)hl; m.block_size = (uint32_t)bs;
        m.flags = (fi[i].block_checksums ? 1u : 0u) | (fi[i].content_checksum ? 2u : 0u);
        m.slot = (uint32_t)slots; m.slot_cap = (uint32_t)cap_blocks; m.skip = 0;
        slots += cap_blocks;
    }
    wc.slots(W, slots, n);
    TRY_RC(upload(c, W, s));
    TRY_HIP(launch_frame_many_walk(in, W.dev(wc.fr), n, W.dev(wc.pay), W.dev(wc.word), W.dev(wc.info), s));
    TRY_HIP(W.fetch(wc.pay, slots, s));
    TRY_HIP(W.fetch(wc.word, slots, s));
    TRY_HIP(W.fetch(wc.info, 8ull * n, s));
    TRY_HIP(hipStreamSynchronize(s));
    return 0;
}

// ---- 3. the batch: compressed blocks (Independent: plain; Linked: chained, level by level), stored blocks (one copy launch)
void ManyDecode::build_batch() {
    std::vector<uint64_t> r_in, r_out, p_off;          // stored blocks; every payload, for the block checksums
    std::vector<uint32_t> r_len, p_len, n_comp(n, 0);
    for (uint32_t i = 0; i < n; i++) {
        if (again[i]) continue;
        const ManyFrame& m = W.host(wc.fr)[i];
        const uint32_t* nf = W.host(wc.info) + 8ull * i;
        if (nf[1] != 0) { again[i] = 1; continue; }                                  // does not parse (bytes behind the frame are not read: read_to_end ends with the frame)
        const uint32_t cnt = nf[0], bs = m.block_size;
        const size_t plain0 = plain.size(), chained0 = chained.size(), r0 = r_in.size(), p0 = p_off.size();
        bool ok = true;
        for (uint32_t k = 0; k < cnt && ok; k++) {
            const uint32_t w = W.host(wc.word)[m.slot + k], len = w & ~BLOCK_UNCOMPRESSED_SIZE_BIT;
            const uint64_t po = W.host(wc.pay)[m.slot + k], pos = (uint64_t)k * bs;
            if (len == 0 || pos >= out_cap[i]) { ok = false; break; }
            const uint32_t cap = (uint32_t)std::min<uint64_t>(bs, out_cap[i] - pos);
            if (m.flags & 1u) { p_off.push_back(po); p_len.push_back(len); p_stream.push_back(i); }
            if (w & BLOCK_UNCOMPRESSED_SIZE_BIT) {
                if (len > cap || (k + 1 != cnt && len != bs)) { ok = false; break; }
                r_in.push_back(po); r_out.push_back(out_off[i] + pos); r_len.push_back(len);
                raw_bytes[i] += len;
            } else {
                Entry e;
                e.stream = i; e.k = k; e.in_off = po; e.in_len = len; e.pos = (uint32_t)pos;
                if (fi[i].block_mode == 1) { e.out_off = out_off[i]; e.cap = (uint32_t)pos + cap; chained.push_back(e); }
                else { e.out_off = out_off[i] + pos; e.cap = cap; e.pos = 0; plain.push_back(e); }
                n_comp[i] += 1;
            }
        }
        if (ok && fi[i].block_mode == 1 && n_comp[i] > CHAIN_MAX_BLOCKS) ok = false;
        if (!ok) {
            again[i] = 1; raw_bytes[i] = 0; n_comp[i] = 0;
            plain.resize(plain0); chained.resize(chained0); r_in.resize(r0); r_out.resize(r0); r_len.resize(r0);
            p_off.resize(p0); p_len.resize(p0); p_stream.resize(p0);
        }
    }
    // chained groups: whole streams, at most CHAIN_MAX_BLOCKS blocks per call, each ordered by (block index, stream)
    {
        size_t lo = 0, at = 0;
        while (at < chained.size()) {
            size_t hi = at;
            const uint32_t st = chained[at].stream;
            while (hi < chained.size() && chained[hi].stream == st) hi++;
            if (hi - lo > CHAIN_MAX_BLOCKS) { groups.push_back({lo, at}); lo = at; }
            at = hi;
        }
        if (chained.size() > lo) groups.push_back({lo, chained.size()});
        for (const Group& g : groups)
            std::stable_sort(chained.begin() + g.lo, chained.begin() + g.hi, [](const Entry& a, const Entry& b) { return a.k < b.k; });
    }
    np = (uint32_t)plain.size(); nc = (uint32_t)chained.size(); nr = (uint32_t)r_in.size(); nk = (uint32_t)p_off.size(); ne = np + nc;
    bc = ManyBatchCols(B, ne, nr, nk, n);
    std::vector<uint32_t> last(n, 0xFFFFFFFFu);        // a stream's latest compressed block in the current group
    auto put = [&](uint32_t at, const Entry& e, uint32_t prev) {
        B.host(bc.in)[at] = e.in_off; B.host(bc.out)[at] = e.out_off; B.host(bc.len)[at] = e.in_len;
        B.host(bc.cap)[at] = e.cap; B.host(bc.pos)[at] = e.pos; B.host(bc.prev)[at] = prev;
    };
    for (uint32_t j = 0; j < np; j++) put(j, plain[j], 0xFFFFFFFFu);
    for (const Group& g : groups)
        for (size_t j = g.lo; j < g.hi; j++) {
            const Entry& e = chained[j];
            put(np + (uint32_t)j, e, last[e.stream]);
            last[e.stream] = (uint32_t)(j - g.lo);                                     // (indices count from the group's first block)
        }
    B.fill(bc.rin, r_in.data()); B.fill(bc.rout, r_out.data()); B.fill(bc.rlen, r_len.data());
    B.fill(bc.poff, p_off.data()); B.fill(bc.plen, p_len.data());
}

int ManyDecode::run_batch() {
    TRY_RC(upload(c, B, s));
    if (nk) {                                          // frame/decompress.rs:255-261,275-278: block checksums, before anything is decoded
        TRY_RC(lz4flex_xxh32_batch_device(in, B.dev(bc.poff), B.dev(bc.plen), nk, 0, B.dev(bc.psum), s));
        TRY_HIP(launch_frame_sums_check(in, B.dev(bc.poff), B.dev(bc.plen), B.dev(bc.psum), nk, B.dev(bc.bad), s));
    }
    if (nr) TRY_RC(lz4flex_copy_batch_device(in, B.dev(bc.rin), B.dev(bc.rlen), out, B.dev(bc.rout), nr, s));   // :262-271
    bool big = false;
    for (const Entry& e : plain) big |= e.in_len > 131072u;
    if (np)
        TRY_RC(lz4flex_decompress_batch(c, in, B.dev(bc.in), B.dev(bc.len), np, out, B.dev(bc.out), B.dev(bc.cap), B.dev(bc.olen), B.dev(bc.st),
                                        B.dev(bc.det), LZ4FLEX_MEM_DEVICE | (big ? LZ4FLEX_MEM_BIG_BLOCKS : 0), s));
    for (const Group& g : groups) {
        const size_t o = np + g.lo;
        lz4flex_decompress_ext ext{};
        ext.out_pos = B.dev(bc.pos) + o;
        ext.chain_prev = B.dev(bc.prev) + o;
        {
            uint32_t chains = 0;                       // (level-by-level order: the blocks without a predecessor are the chains)
            for (size_t j = g.lo; j < g.hi; j++) chains += B.host(bc.prev)[np + j] == 0xFFFFFFFFu ? 1u : 0u;
            ext.n_chains = chains;
        }
        const int level_min = lz4flex_get_tuning(c, "decompress_level_chains");
        if (level_min > 0 && ext.n_chains >= (uint32_t)level_min) {
            // MANY short chains (round 6): a LEVEL per launch -- block k of every stream, a plain batch with prefixes (out_pos) whose bytes the
            // launches before it have written: the batch decoders by batch shape (the sequence decoder from 641 blocks on: 4 096 chains of
            // 4 blocks 6.7 -> 2.3 ms per GiB) instead of one workgroup per block polling its predecessor.  A level costs ~0.3 ms whatever it
            // holds, so this is for thousands of chains; hundreds of long ones (256 x 64 blocks) stay with the chained launch
            for (size_t j = g.lo; j < g.hi;) {
                size_t e = j;
                while (e < g.hi && chained[e].k == chained[j].k) e++;
                const size_t oj = np + j;
                lz4flex_decompress_ext lv{};
                lv.out_pos = B.dev(bc.pos) + oj;
                TRY_RC(lz4flex_decompress_batch_ex(c, in, B.dev(bc.in) + oj, B.dev(bc.len) + oj, (uint32_t)(e - j), out, B.dev(bc.out) + oj, B.dev(bc.cap) + oj,
                                                   B.dev(bc.olen) + oj, B.dev(bc.st) + oj, B.dev(bc.det) + 2 * oj, &lv, LZ4FLEX_MEM_DEVICE, s));
                j = e;
            }
            continue;
        }
        TRY_RC(lz4flex_decompress_batch_ex(c, in, B.dev(bc.in) + o, B.dev(bc.len) + o, (uint32_t)(g.hi - g.lo), out, B.dev(bc.out) + o, B.dev(bc.cap) + o,
                                           B.dev(bc.olen) + o, B.dev(bc.st) + o, B.dev(bc.det) + 2 * o, &ext, LZ4FLEX_MEM_DEVICE | LZ4FLEX_MEM_CHAINED, s));
    }
    TRY_HIP(B.fetch(bc.olen, ne, s));
    TRY_HIP(B.fetch(bc.st, ne, s));
    TRY_HIP(B.fetch(bc.bad, nk, s));
    TRY_HIP(hipStreamSynchronize(s));
    return 0;
}

// ---- 4. verdicts and content checksums, then the streams that go through decompress_one
int ManyDecode::finish(uint64_t* out_len, int32_t* status, lz4flex_err_detail* detail) {
    std::vector<uint64_t> produced(raw_bytes);
    for (uint32_t j = 0; j < nk; j++) if (B.host(bc.bad)[j]) again[p_stream[j]] = 1;
    auto judge = [&](const Entry& e, uint32_t at) {
        const uint32_t i = e.stream;
        const ManyFrame& m = W.host(wc.fr)[i];
        const uint32_t cnt = W.host(wc.info)[8ull * i], got = B.host(bc.olen)[at];
        if (B.host(bc.st)[at] != 0 || (e.k + 1 != cnt && got != m.block_size)) again[i] = 1;   // an error; a short block inside the frame (flush())
        produced[i] += got;
    };
    for (uint32_t j = 0; j < np; j++) judge(plain[j], j);
    for (uint32_t j = 0; j < nc; j++) judge(chained[j], np + j);
    // content size and checksum (frame/decompress.rs:205-229)
    std::vector<uint32_t> cs;                          // streams whose content checksum is being computed
    for (uint32_t i = 0; i < n; i++) {
        if (again[i]) continue;
        if (fi[i].has_content_size && fi[i].content_size != produced[i]) { again[i] = 1; continue; }
        if (fi[i].content_checksum) {
            if (produced[i] > 0xFFFFFFFFull) { again[i] = 1; continue; }
            B.host(bc.coff)[cs.size()] = out_off[i]; B.host(bc.clen)[cs.size()] = (uint32_t)produced[i];
            cs.push_back(i);
        }
    }
    if (!cs.empty()) {
        const uint32_t m = (uint32_t)cs.size();
        TRY_HIP(hipMemcpyAsync(B.dev(bc.coff), B.host(bc.coff), 8ull * m, hipMemcpyHostToDevice, s));
        TRY_HIP(hipMemcpyAsync(B.dev(bc.clen), B.host(bc.clen), 4ull * m, hipMemcpyHostToDevice, s));
        TRY_RC(lz4flex_xxh32_batch_device(out, B.dev(bc.coff), B.dev(bc.clen), m, 0, B.dev(bc.csum), s));
        TRY_HIP(B.fetch(bc.csum, m, s));
        TRY_HIP(hipStreamSynchronize(s));
        for (uint32_t j = 0; j < m; j++)
            if (B.host(bc.csum)[j] != W.host(wc.info)[8ull * cs[j] + 4]) again[cs[j]] = 1;
    }
    for (uint32_t i = 0; i < n; i++) {
        if (detail) memset(&detail[i], 0, sizeof detail[i]);
        if (!again[i]) { status[i] = 0; out_len[i] = produced[i]; continue; }
        TRY_RC(decompress_one(in + in_off[i], in_len[i], out + out_off[i], out_cap[i], &out_len[i], &status[i], detail ? &detail[i] : nullptr, s));
    }
    return 0;
}

int decompress_many_device(lz4flex_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n, uint8_t* out,
                           const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status, lz4flex_err_detail* detail,
                           hipStream_t s) {
    ManyDecode m(ManyArgs{c, in, in_off, in_len, n, out, out_off, out_cap, s});
    TRY_RC(m.read_heads());
    TRY_RC(m.walk_tables());
    m.build_batch();
    TRY_RC(m.run_batch());
    return m.finish(out_len, status, detail);
}

// ---- host buffers: staged through device scratch (slots 2 and 3), then the device path
uint64_t staged(const uint64_t* len, uint32_t n, std::vector<uint64_t>& off) {
    uint64_t at = 0;
    off.resize(n);
    for (uint32_t i = 0; i < n; i++) { off[i] = at; at += (len[i] + 255) / 256 * 256; }
    return at;
}

}  // namespace

extern "C" {

int lz4flex_frame_compress_many(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint64_t* in_len, uint32_t n,
                                const lz4flex_frame_info* info, void* out_base, const uint64_t* out_off, const uint64_t* out_cap,
                                uint64_t* out_len, int32_t* status, int mem_kind, void* hip_stream) {
    if (n == 0) return 0;
    if (!in_off || !in_len || !out_off || !out_cap || !out_len || !status || !out_base) return -LZ4FLEX_E_INVALID_ARG;
    TRY_RC(ctx_resolve(&ctx));
    lz4flex_frame_info def{};
    if (!info) info = &def;                                                             // FrameInfo::default(), frame/header.rs:151-163
    if (info->legacy_frame) return -LZ4FLEX_E_INVALID_ARG;
    try {
    if (mem_kind != LZ4FLEX_MEM_HOST && mem_kind != LZ4FLEX_MEM_DEVICE) return -LZ4FLEX_E_INVALID_ARG;
    // (the DEVICE path too: the call's scratch is allocated on -- and cached with -- the context's device, whatever the thread's current one is)
    DeviceGuard guard(ctx->device);
    if (mem_kind == LZ4FLEX_MEM_DEVICE)
        return compress_many_device(ctx, (const uint8_t*)in_base, in_off, in_len, n, info, (uint8_t*)out_base, out_off, out_cap, out_len, status,
                                    (hipStream_t)hip_stream);
    hipStream_t s = ctx->stream;
    std::vector<uint64_t> s_in, s_out, cap(n);
    for (uint32_t i = 0; i < n; i++) cap[i] = std::min<uint64_t>(out_cap[i], lz4flex_frame_compress_bound((size_t)in_len[i], info));
    const uint64_t in_bytes = staged(in_len, n, s_in), out_bytes = staged(cap.data(), n, s_out);
    void *d_in = nullptr, *d_out = nullptr;
    TRY_RC(ctx_scratch(ctx, 2, (size_t)in_bytes + 64, &d_in));
    TRY_RC(ctx_scratch(ctx, 3, (size_t)out_bytes + 64, &d_out));
    for (uint32_t i = 0; i < n; i++)
        if (in_len[i]) TRY_HIP(hipMemcpyAsync((uint8_t*)d_in + s_in[i], (const uint8_t*)in_base + in_off[i], (size_t)in_len[i], hipMemcpyHostToDevice, s));
    TRY_RC(compress_many_device(ctx, (const uint8_t*)d_in, s_in.data(), in_len, n, info, (uint8_t*)d_out, s_out.data(), cap.data(), out_len, status, s));
    for (uint32_t i = 0; i < n; i++)
        if (status[i] == 0 && out_len[i]) TRY_HIP(hipMemcpyAsync((uint8_t*)out_base + out_off[i], (const uint8_t*)d_out + s_out[i], (size_t)out_len[i], hipMemcpyDeviceToHost, s));
    TRY_HIP(hipStreamSynchronize(s));
    return 0;
    } catch (const std::bad_alloc&) { return -LZ4FLEX_E_NOMEM; }      // (host tables and staging are std::vectors: nothing escapes the C ABI)
      catch (...) { return -LZ4FLEX_E_NOMEM; }                         // (std::length_error of an absurd size)
}

int lz4flex_frame_decompress_many(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint64_t* in_len, uint32_t n,
                                  void* out_base, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status,
                                  lz4flex_err_detail* detail, int mem_kind, void* hip_stream) {
    if (n == 0) return 0;
    if (!in_off || !in_len || !out_off || !out_cap || !out_len || !status || !in_base) return -LZ4FLEX_E_INVALID_ARG;
    TRY_RC(ctx_resolve(&ctx));
    try {
    if (mem_kind != LZ4FLEX_MEM_HOST && mem_kind != LZ4FLEX_MEM_DEVICE) return -LZ4FLEX_E_INVALID_ARG;
    DeviceGuard guard(ctx->device);
    if (mem_kind == LZ4FLEX_MEM_DEVICE)
        return decompress_many_device(ctx, (const uint8_t*)in_base, in_off, in_len, n, (uint8_t*)out_base, out_off, out_cap, out_len, status, detail,
                                      (hipStream_t)hip_stream);
    hipStream_t s = ctx->stream;
    std::vector<uint64_t> s_in, s_out;
    const uint64_t in_bytes = staged(in_len, n, s_in), out_bytes = staged(out_cap, n, s_out);
    void *d_in = nullptr, *d_out = nullptr;
    TRY_RC(ctx_scratch(ctx, 2, (size_t)in_bytes + 64, &d_in));
    TRY_RC(ctx_scratch(ctx, 3, (size_t)out_bytes + 64, &d_out));
    for (uint32_t i = 0; i < n; i++)
        if (in_len[i]) TRY_HIP(hipMemcpyAsync((uint8_t*)d_in + s_in[i], (const uint8_t*)in_base + in_off[i], (size_t)in_len[i], hipMemcpyHostToDevice, s));
    TRY_RC(decompress_many_device(ctx, (const uint8_t*)d_in, s_in.data(), in_len, n, (uint8_t*)d_out, s_out.data(), out_cap, out_len, status, detail, s));
    for (uint32_t i = 0; i < n; i++)
        if (status[i] == 0 && out_len[i]) TRY_HIP(hipMemcpyAsync((uint8_t*)out_base + out_off[i], (const uint8_t*)d_out + s_out[i], (size_t)out_len[i], hipMemcpyDeviceToHost, s));
    TRY_HIP(hipStreamSynchronize(s));
    return 0;
    } catch (const std::bad_alloc&) { return -LZ4FLEX_E_NOMEM; }
      catch (...) { return -LZ4FLEX_E_NOMEM; }
}

}  // extern "C"
