// frame.cpp -- host side of the LZ4 frame layer (lz4_flex::frame::{FrameEncoder, FrameDecoder,
// FrameInfo}; reference src/frame/{compress,decompress,header}.rs).  Header (de)serialisation,
// block framing, store-raw rule, checksums and the io::Write / io::Read behaviour live here;
// every block's bytes are produced by the batched HIP kernels through the C ABI.  Where the
// reference calls the block codec once per block (src/frame/compress.rs:282-298,
// src/frame/decompress.rs:288-305) this layer gathers up to `batch_blocks` blocks per launch (the integer rules: frame_plan.h).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/lz4flex_amd.h"
#include "frame_plan.h"
#include "host_pin.h"
#include "lz4_batch_entry.h"
#include "xxh32.h"

namespace {

using lz4flex::PinBuf;
using lz4flex::XxHash32;
using namespace lz4flex_plan;   // block sizes, BLOCK_UNCOMPRESSED_SIZE_BIT, WINDOW_SIZE, TableOffset, LinkedWindow, DecodeRing, DecodeRuns

// src/frame/header.rs:11-34
constexpr uint8_t FLG_RESERVED_MASK = 0x02, FLG_VERSION_MASK = 0xC0, FLG_SUPPORTED_VERSION_BITS = 0x40,
                  FLG_INDEPENDENT_BLOCKS = 0x20, FLG_BLOCK_CHECKSUMS = 0x10, FLG_CONTENT_SIZE = 0x08,
                  FLG_CONTENT_CHECKSUM = 0x04, FLG_DICTIONARY_ID = 0x01, BD_BLOCK_SIZE_MASK = 0x70,
                  BD_RESERVED_MASK = 0x8F;
constexpr uint32_t LZ4F_MAGIC_NUMBER = 0x184D2204u, LZ4F_LEGACY_MAGIC_NUMBER = 0x184C2102u;
constexpr size_t MIN_FRAME_INFO_SIZE = 7, MAX_FRAME_INFO_SIZE = 19;

uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
uint64_t rd64(const uint8_t* p) { return (uint64_t)rd32(p) | ((uint64_t)rd32(p + 4) << 32); }
void wr32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
void wr64(uint8_t* p, uint64_t v) { wr32(p, (uint32_t)v); wr32(p + 4, (uint32_t)(v >> 32)); }

// FrameEncoder: the stream bytes [base, base + len) that wait for a launch or are the history of the blocks to come; page-locked (host_pin.h)
struct Stage {
    PinBuf buf;
    size_t len = 0;
    uint64_t base = 0;             // stream position of buf[0]
    const uint8_t* at(uint64_t pos) const { return buf.data() + (size_t)(pos - base); }
    // grows with the data, by doubling, to at most `limit` bytes
    void append(const uint8_t* p, size_t n, size_t limit) {
        if (buf.size() < len + n) buf.resize(std::min(limit, std::max(buf.size() * 2, len + n)));
        memcpy(buf.data() + len, p, n);
        len += n;
    }
    // forgets what lies in front of stream position `pos`
    void drop_before(uint64_t pos) {
        if (pos <= base) return;
        const size_t drop = (size_t)(pos - base);
        memmove(buf.data(), buf.data() + drop, len - drop);
        len -= drop; base = pos;
    }
};

// FrameEncoder: the block columns of one launch and the compressed slots they name, at a fixed stride
struct EncodeBatch {
    PinBuf dst;
    std::vector<uint64_t> in_off, out_off;
    std::vector<uint32_t> in_len, out_cap, out_len, flags;
    std::vector<int32_t> status;
    std::vector<lz4flex_chain_block> chain;
    // `total` bytes at offset `first` of the launch's source, as blocks of `mbs` (the last may be partial): returns their number
    size_t prepare(size_t total, size_t mbs, size_t first) {
        const size_t nblk = (total + mbs - 1) / mbs, stride = slot_stride(mbs);
        if (dst.size() < stride * nblk) dst.resize(stride * nblk);
        in_off.resize(nblk); in_len.resize(nblk); flags.resize(nblk); out_off.resize(nblk); out_cap.resize(nblk); out_len.resize(nblk); status.resize(nblk);
        for (size_t i = 0; i < nblk; i++) {
            in_off[i] = first + i * mbs; in_len[i] = (uint32_t)std::min(mbs, total - i * mbs);
            out_off[i] = i * stride; out_cap[i] = (uint32_t)stride;
        }
        return nblk;
    }
};

}  // namespace

extern "C" {

uint32_t lz4flex_xxh32(const uint8_t* data, size_t len, uint32_t seed) { return XxHash32::oneshot(seed, data, len); }

// FrameInfo::write, header.rs:232-275
int64_t lz4flex_frame_info_write(const lz4flex_frame_info* fi, uint8_t* out, size_t out_cap) {
    if (!fi || !out) return -LZ4FLEX_E_INVALID_ARG;
    const size_t write_size = MIN_FRAME_INFO_SIZE + (fi->has_content_size ? 8 : 0);
    if (out_cap < write_size) return -LZ4FLEX_FE_IO;
    uint8_t b[MAX_FRAME_INFO_SIZE] = {0};
    wr32(b, LZ4F_MAGIC_NUMBER);
    b[4] = FLG_SUPPORTED_VERSION_BITS;
    if (fi->block_checksums) b[4] |= FLG_BLOCK_CHECKSUMS;
    if (fi->content_checksum) b[4] |= FLG_CONTENT_CHECKSUM;
    if (fi->block_mode == 0) b[4] |= FLG_INDEPENDENT_BLOCKS;
    b[5] = (uint8_t)(fi->block_size << 4);
    size_t off = 6;
    if (fi->has_content_size) { b[4] |= FLG_CONTENT_SIZE; wr64(b + off, fi->content_size); off += 8; }
    b[off] = (uint8_t)(XxHash32::oneshot(0, b + 4, off - 4) >> 8);
    memcpy(out, b, write_size);
    return (int64_t)write_size;
}

// FrameInfo::read, header.rs:277-373
int64_t lz4flex_frame_info_read(const uint8_t* in, size_t in_len, lz4flex_frame_info* fi, lz4flex_err_detail* d) {
    if (!in || !fi) return -LZ4FLEX_E_INVALID_ARG;
    memset(fi, 0, sizeof *fi);
    if (in_len < 4) return -LZ4FLEX_FE_IO;
    const uint32_t magic = rd32(in);
    size_t p = 4;
    if (magic == LZ4F_LEGACY_MAGIC_NUMBER) { fi->block_size = 8; fi->legacy_frame = 1; return 4; }
    if (magic >= 0x184D2A50u && magic <= 0x184D2A5Fu) {
        if (in_len < 8) return -LZ4FLEX_FE_IO;
        if (d) d->expected = rd32(in + 4);
        return -LZ4FLEX_FE_SKIPPABLE_FRAME;
    }
    if (magic != LZ4F_MAGIC_NUMBER) return -LZ4FLEX_FE_WRONG_MAGIC;
    if (in_len < p + 2) return -LZ4FLEX_FE_IO;
    const uint8_t flg = in[p], bd = in[p + 1];
    p += 2;
    if ((flg & FLG_VERSION_MASK) != FLG_SUPPORTED_VERSION_BITS) {
        if (d) d->expected = flg & FLG_VERSION_MASK;
        return -LZ4FLEX_FE_UNSUPPORTED_VERSION;
    }
    if ((flg & FLG_RESERVED_MASK) || (bd & BD_RESERVED_MASK)) return -LZ4FLEX_FE_RESERVED_BITS;
    fi->block_mode = (flg & FLG_INDEPENDENT_BLOCKS) ? 0 : 1;
    fi->content_checksum = (flg & FLG_CONTENT_CHECKSUM) != 0;
    fi->block_checksums = (flg & FLG_BLOCK_CHECKSUMS) != 0;
    const int bs = (bd & BD_BLOCK_SIZE_MASK) >> 4;
    if (bs <= 3) { if (d) d->expected = (uint64_t)bs; return -LZ4FLEX_FE_UNSUPPORTED_BLOCKSIZE; }
    fi->block_size = bs;
    if (flg & FLG_CONTENT_SIZE) {
        if (in_len < p + 8) return -LZ4FLEX_FE_IO;
        fi->has_content_size = 1; fi->content_size = rd64(in + p); p += 8;
    }
    bool has_dict = false;
    if (flg & FLG_DICTIONARY_ID) { if (in_len < p + 4) return -LZ4FLEX_FE_IO; has_dict = true; p += 4; }
    if (in_len < p + 1) return -LZ4FLEX_FE_IO;
    if ((uint8_t)(XxHash32::oneshot(0, in + 4, p - 4) >> 8) != in[p]) return -LZ4FLEX_FE_HEADER_CHECKSUM;
    p += 1;
    if (has_dict) return -LZ4FLEX_FE_DICTIONARY_NOT_SUPPORTED;   // frame/decompress.rs:139-142
    return (int64_t)p;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// FrameEncoder
struct lz4flex_frame_encoder {
    lz4flex_frame_info fi{};
    lz4flex_write_fn w = nullptr;
    void* user = nullptr;
    Stage stage;                   // Independent: the bytes not yet compressed; Linked: the history the blocks to come can reach in front of them
    EncodeBatch b;
    size_t batch_blocks = 0;       // blocks per kernel launch
    size_t batch_bytes = 64u << 20;
    bool batch_auto = true;        // no explicit set_batch_bytes: big blocks get enough blocks per launch to fill the GPU
    uint64_t content_len = 0;
    TableOffset tbl;               // Independent frame: mirrors the reference field that decides the table state (N3)
    XxHash32 content_hasher{0};
    bool is_frame_open = false, data_to_frame_written = false;
    bool final_write = false;       // lz4flex_frame_compress: the write in progress is the stream's last (finish follows)
    int sticky_err = 0;
    uint64_t proc_pos = 0;              // stream position of the first byte not yet compressed
    uint64_t frame_start = 0;           // stream position of the current frame's first byte (history never reaches before it)
    // Linked mode (frame/compress.rs:62-93): the reference's src ring (prefix + ext_dict) expressed in
    // stream coordinates (`win`); the dependent blocks of a batch run as ONE chain on the GPU.
    LinkedWindow win;
    std::vector<uint32_t> tbl_state;    // the persistent HashTable4K
    bool linked_fast = false;           // Linked frame written with the throughput encoder: blocks parsed independently

    int emit(const uint8_t* p, size_t n) {
        while (n) {
            const int64_t k = w(user, p, n);
            if (k <= 0) return -LZ4FLEX_FE_IO;     // io::ErrorKind::WriteZero / other
            p += (size_t)k; n -= (size_t)k;
        }
        return 0;
    }
    // begin_frame, frame/compress.rs:234-257 (+ init :96-118)
    int begin_frame(size_t buf_len) {
        is_frame_open = true;
        if (fi.block_size == 0) fi.block_size = block_size_from_buf_length(buf_len);
        const size_t mbs = block_size_bytes(fi.block_size);
        if (mbs == 0 || fi.block_size == 8) return -LZ4FLEX_E_INVALID_ARG;   // Max8MB is legacy-decode only (header.rs:287)
        batch_blocks = blocks_per_launch(batch_bytes, mbs, batch_auto);
        uint8_t hdr[MAX_FRAME_INFO_SIZE];
        const int64_t n = lz4flex_frame_info_write(&fi, hdr, sizeof hdr);
        if (n < 0) return (int)n;
        int rc = emit(hdr, (size_t)n);
        if (rc) return rc;
        if (content_len != 0) {   // second or later frame of this encoder: reset compressor state
            content_len = 0; tbl.so = 0;       // (nothing is staged between frames: try_finish flushed; a Linked frame's history
            content_hasher.reset(0);           // stays where it is, out of the new frame's reach: win, frame_start)
            win.reset(proc_pos);
            std::fill(tbl_state.begin(), tbl_state.end(), 0u);
        }
        if (fi.block_mode == 1 && tbl_state.empty()) tbl_state.assign(4096, 0u);
        linked_fast = fi.block_mode == 1 && lz4flex_get_tuning(nullptr, "compress_mode") != 1;   // decided once per frame
        frame_start = proc_pos;
        return 0;
    }
    // One block's bytes on the wire (frame/compress.rs:301-321): BlockInfo, payload (the source itself where compression did
    // not help), optional block checksum; content hash and length move on
    int emit_block(const uint8_t* s, size_t slen, const uint8_t* comp_bytes, uint32_t comp_len) {
        const uint8_t* block_data; size_t block_len; uint32_t info;
        if (comp_len < slen) { block_data = comp_bytes; block_len = comp_len; info = comp_len; }                      // :301-306
        else { block_data = s; block_len = slen; info = (uint32_t)slen | BLOCK_UNCOMPRESSED_SIZE_BIT; }
        uint8_t bi[4]; wr32(bi, info);
        int rc;
        if ((rc = emit(bi, 4))) return rc;
        if ((rc = emit(block_data, block_len))) return rc;
        if (fi.block_checksums) {                                                                                      // :313-316
            uint8_t c[4]; wr32(c, XxHash32::oneshot(0, block_data, block_len));
            if ((rc = emit(c, 4))) return rc;
        }
        if (fi.content_checksum) content_hasher.write(s, slen);                                                        // :319-321
        content_len += slen;
        return 0;
    }
    // the blocks of a launch that went through, on the wire; `src`: what the batch's in_off count from
    int emit_batch(const uint8_t* src, size_t nblk) {
        for (size_t i = 0; i < nblk; i++) {
            if (b.status[i] != 0) return -LZ4FLEX_FE_COMPRESSION;
            const int rc = emit_block(src + b.in_off[i], b.in_len[i], b.dst.data() + b.out_off[i], b.out_len[i]);
            if (rc) return rc;
        }
        return 0;
    }

    // write_block (frame/compress.rs:261-371) for the `total` bytes at proc_pos in one launch, as blocks of <= block_size in order; the last
    // may be partial.  Three forms: each fills what its entry point reads, calls it, and says what stays staged as history.
    // Independent frame.  The blocks are the staged bytes, or (round 6) `direct`, bytes in the CALLER's buffer: a write of a whole batch, and the
    // one-shot call's remainder, are compressed where they lie -- staging them cost a host copy of every byte (12 instead of 24 GiB/s
    // through host buffers).  Nothing is history.
    int write_blocks(size_t total, const uint8_t* direct = nullptr) {
        const uint8_t* const src = direct ? direct : stage.at(proc_pos);
        const size_t mbs = block_size_bytes(fi.block_size), nblk = b.prepare(total, mbs, 0);
        TableOffset t = tbl;             // (committed below, once the launch and every write went through)
        for (size_t i = 0; i < nblk; i++) b.flags[i] = t.next(mbs, b.in_len[i]);
        int rc = lz4flex_compress_batch(nullptr, src, b.in_off.data(), b.in_len.data(), b.flags.data(), (uint32_t)nblk,
                                        b.dst.data(), b.out_off.data(), b.out_cap.data(), b.out_len.data(), b.status.data(),
                                        LZ4FLEX_MEM_HOST, nullptr);
        if (rc || (rc = emit_batch(src, nblk))) return rc;
        tbl = t;
        proc_pos += total;
        if (direct) stage.base = proc_pos; else stage.drop_before(proc_pos);      // (direct: the stage is empty and stays so)
        return 0;
    }
    // Linked frame, throughput encoder (compress_mode fast): a block's matches reach into the 32 KiB of the stream in front of it
    // (LZ4FLEX_BLOCK_HISTORY: the history is INPUT, so the blocks of a launch are still one batch and not one dependency chain
    // -- 64 blocks of 64 KiB: one launch of a fraction of a millisecond instead of 64 x 8 ms of chain).  Any LZ4 frame decoder
    // returns the input; JSON, 64 KiB blocks: ratio 0.2216 (the reference's Linked frame 0.2226, independent blocks 0.2307).
    // compress_mode exact keeps the reference's bytes (write_blocks_linked below).
    int write_blocks_linked_fast(size_t total) {
        const size_t mbs = block_size_bytes(fi.block_size), nblk = b.prepare(total, mbs, (size_t)(proc_pos - stage.base));
        for (size_t i = 0; i < nblk; i++) {
            // what the stage holds in front of the block, as far as it belongs to THIS frame
            const uint64_t have = std::min<uint64_t>(b.in_off[i], proc_pos + i * mbs - frame_start);
            b.flags[i] = LZ4FLEX_BLOCK_HISTORY(std::min<uint64_t>(have, FAST_HISTORY));
        }
        // (a Linked frame's blocks: what compress_mode high does with them is encode_route's rule, lz4_route.h)
        int rc = lz4flex_dev::compress_batch_entry(nullptr, stage.buf.data(), b.in_off.data(), b.in_len.data(), b.flags.data(), (uint32_t)nblk,
                                                   b.dst.data(), b.out_off.data(), b.out_cap.data(), b.out_len.data(), b.status.data(),
                                                   LZ4FLEX_MEM_HOST, nullptr, true);
        if (rc || (rc = emit_batch(stage.buf.data(), nblk))) return rc;
        proc_pos += total;
        stage.drop_before(proc_pos >= FAST_HISTORY ? proc_pos - FAST_HISTORY : 0);   // the next block's history stays
        return 0;
    }
    // Linked frame, the reference's bytes: the blocks are ONE chain on the device, with the reference's window bookkeeping
    // (frame/compress.rs:261-371) done in stream coordinates (`win` moves on before the launch)
    int write_blocks_linked(size_t total) {
        const size_t mbs = block_size_bytes(fi.block_size), nblk = b.prepare(total, mbs, (size_t)(proc_pos - stage.base));
        b.chain.resize(nblk);
        for (size_t i = 0; i < nblk; i++) {
            lz4flex_chain_block& c = b.chain[i];
            c = win.next(mbs, b.in_len[i]);                  // (stream positions; the stage starts at stage.base)
            c.in_off -= stage.base;
            if (c.dict_len) c.dict_off -= stage.base;
        }
        const uint32_t first = 0, count = (uint32_t)nblk;
        int rc = lz4flex_compress_chains(nullptr, stage.buf.data(), b.chain.data(), (uint32_t)nblk, &first, &count, 1, b.dst.data(),
                                         b.out_off.data(), b.out_cap.data(), b.out_len.data(), b.status.data(), tbl_state.data(),
                                         LZ4FLEX_MEM_HOST, nullptr);
        if (rc || (rc = emit_batch(stage.buf.data(), nblk))) return rc;
        proc_pos += total;
        stage.drop_before(win.keep_from());                  // drop history the window can no longer reach
        return 0;
    }
    size_t pending() const { return (size_t)(stage.base + stage.len - proc_pos); }   // staged and not yet compressed
    int write_pending() {
        const size_t n = pending();
        if (n == 0) return 0;
        return fi.block_mode != 1 ? write_blocks(n) : linked_fast ? write_blocks_linked_fast(n) : write_blocks_linked(n);
    }
    // io::Write::write, frame/compress.rs:375-396
    int64_t write(const uint8_t* buf, size_t len) {
        if (sticky_err) return sticky_err;
        int rc;
        if (!is_frame_open && len != 0) { if ((rc = begin_frame(len))) return sticky_err = rc; }
        const bool linked = fi.block_mode == 1;
        const size_t total = len, mbs = block_size_bytes(fi.block_size);
        // (exact-mode Linked: the blocks of a launch are ONE dependency chain on the device -- 64 of them keep a launch in the tens of
        // milliseconds; everything else: independent blocks, a full batch per launch)
        const size_t cap = (linked && !linked_fast ? std::min<size_t>(batch_blocks, 64) : batch_blocks) * mbs;
        while (len) {
            if (pending() == cap) { if ((rc = write_pending())) return sticky_err = rc; continue; }   // staging full: the staged blocks make space
            // No staging: a whole batch lies in the caller's buffer; or this is the one-shot call's remainder -- whatever is left is the
            // frame's end, a partial last block included
            if (!linked && pending() == 0 && (len >= cap || final_write)) {
                const size_t n = std::min(cap, len);
                if ((rc = write_blocks(n, buf))) return sticky_err = rc;
                buf += n; len -= n;
                continue;
            }
            const size_t n = std::min(cap - pending(), len);
            stage.append(buf, n, linked ? (size_t)-1 : cap);   // (Independent: never more than a batch)
            buf += n; len -= n;
        }
        return (int64_t)total;
    }
    // io::Write::flush, frame/compress.rs:398-403
    int flush() {
        if (sticky_err) return sticky_err;
        const int rc = write_pending();
        return rc ? (sticky_err = rc) : 0;
    }
    // try_finish, frame/compress.rs:173-187 (+ end_frame :209-230)
    int try_finish(lz4flex_err_detail* d) {
        int rc = flush();
        if (rc) return rc;
        if (!is_frame_open && !data_to_frame_written) { if ((rc = begin_frame(0))) return rc; }
        is_frame_open = false;
        if (fi.has_content_size && fi.content_size != content_len) {
            if (d) { d->expected = fi.content_size; d->actual = content_len; }
            return -LZ4FLEX_FE_CONTENT_LENGTH;
        }
        uint8_t z[4] = {0, 0, 0, 0};
        if ((rc = emit(z, 4))) return rc;
        if (fi.content_checksum) {
            uint8_t c[4]; wr32(c, content_hasher.finish());
            if ((rc = emit(c, 4))) return rc;
        }
        data_to_frame_written = true;
        return 0;
    }
};

// ------------------------------------------------------------------------------------------
// FrameDecoder
struct lz4flex_frame_decoder {
    lz4flex_read_fn r = nullptr;
    void* user = nullptr;
    bool have_frame = false;
    lz4flex_frame_info fi{};
    XxHash32 content_hasher{0};
    uint64_t content_len = 0;
    size_t batch_bytes = 64u << 20;
    bool batch_auto = true;
    PinBuf comp, out;          // the staged batch; page-locked (host_pin.h)
    std::vector<uint64_t> in_off, out_off, detail;
    std::vector<uint32_t> in_len, out_cap, out_len;
    std::vector<int32_t> status;
    // a gathered block: stored or compressed, its payload comp[at, at + len), `end` = in_total behind it, col: its place in the launch's
    // columns (compressed blocks), out_at: where its sink starts in the launch's output
    struct Slot { bool raw; size_t at, len, end, col, out_at; };
    std::vector<Slot> slots;
    size_t out_need = 0;       // bytes of output the gathered blocks were given
    bool saw_end = false;      // the gathering stopped at the EndMark
    struct Item { size_t off, len, src_end; };   // decoded bytes waiting to be read: offsets into `out` (Independent) or `ldst` (Linked)
    std::vector<Item> ready;   // decoded pieces in stream order (len 0 = a block that decoded to nothing; src_end: the input read up to its end)
    size_t ready_idx = 0, ready_pos = 0;
    bool ready_linked = false; // the ready items index `ldst` (a Linked frame's blocks stay where they were decoded)
    int pending_err = 0;       // surfaces after the pieces before it were delivered
    lz4flex_err_detail pending_detail{};
    bool pending_zero = false; // EndMark reached: one read() returns 0
    PinBuf ldst;               // Linked: [the frame's last <= 64 KiB | what the last call produced], grown on demand, never shrunk
    size_t lhave = 0;          // Linked: valid bytes in ldst
    DecodeRing ring;           // Linked: the reference's dst ring, for the sink of a block and an OutputTooSmall's positions; the bytes live in ldst
    size_t in_total = 0;           // bytes taken from the reader
    size_t zero_end = (size_t)-1;  // in_total behind the empty block that made the last read return 0 (lz4flex_frame_decompress: *consumed)
    bool io_failed = false;    // the read callback itself reported an error (not a short read)
    static constexpr size_t DIRECT_MIN = 1u << 20;    // a reader with less room than this gets its bytes from the staging buffer (small reads: one launch per read would cost more than the copy)

    // read_exact; returns 0 ok, 1 clean EOF before any byte, -code on short read / error
    int read_exact(uint8_t* p, size_t n, size_t* got_out = nullptr) {
        size_t got = 0;
        while (got < n) {
            const int64_t k = r(user, p + got, n - got);
            if (k < 0) { io_failed = true; in_total += got; return -LZ4FLEX_FE_IO; }
            if (k == 0) break;
            got += (size_t)k;
        }
        in_total += got;
        if (got_out) *got_out = got;
        if (got == n) return 0;
        return got == 0 ? 1 : -LZ4FLEX_FE_IO;
    }
    // read_frame_info, frame/decompress.rs:109-168. 1 = EOF (Ok(0)), 0 = frame opened, <0 error
    int read_frame_info(lz4flex_err_detail* d) {
        uint8_t b[MAX_FRAME_INFO_SIZE];
        int rc = read_exact(b, 4);
        if (rc) return rc;
        size_t required;
        const uint32_t magic = rd32(b);
        if (magic == LZ4F_LEGACY_MAGIC_NUMBER) {
            required = 4;
        } else {
            rc = read_exact(b + 4, MIN_FRAME_INFO_SIZE - 4);
            if (rc) return rc;   // 1: r.read() returned 0 => Ok(0)
            // FrameInfo::read_size, header.rs:194-219
            if (magic >= 0x184D2A50u && magic <= 0x184D2A5Fu) required = 8;
            else if (magic != LZ4F_MAGIC_NUMBER) return -LZ4FLEX_FE_WRONG_MAGIC;
            else required = MIN_FRAME_INFO_SIZE + ((b[4] & FLG_CONTENT_SIZE) ? 8 : 0) + ((b[4] & FLG_DICTIONARY_ID) ? 4 : 0);
            if (required != MIN_FRAME_INFO_SIZE) {
                rc = read_exact(b + MIN_FRAME_INFO_SIZE, required - MIN_FRAME_INFO_SIZE);
                if (rc) return rc == 1 ? -LZ4FLEX_FE_IO : rc;
            }
        }
        const int64_t hs = lz4flex_frame_info_read(b, required, &fi, d);
        if (hs < 0) return (int)hs;
        have_frame = true;
        content_hasher.reset(0);
        content_len = 0;
        ring.reset(); lhave = 0;
        return 0;
    }
    const uint8_t* ready_base() const { return (ready_linked ? ldst : out).data(); }
    void fail(int code, const lz4flex_err_detail* d = nullptr) {
        pending_err = code;
        if (d) pending_detail = *d; else memset(&pending_detail, 0, sizeof pending_detail);
    }
    // what the kernels said about the launch's block `i`, as a DecompressionError's detail
    lz4flex_err_detail block_detail(size_t i) const {
        lz4flex_err_detail d{}; d.expected = detail[2 * i]; d.actual = detail[2 * i + 1]; d.inner = status[i]; return d;
    }
    void fail_block(const lz4flex_err_detail& d) { fail(-LZ4FLEX_FE_DECOMPRESSION, &d); pending_zero = false; }
    // EndMark handling, frame/decompress.rs:313-332
    void end_mark() {
        if (fi.has_content_size && content_len != fi.content_size) {
            lz4flex_err_detail d{}; d.expected = fi.content_size; d.actual = content_len;
            fail(-LZ4FLEX_FE_CONTENT_LENGTH, &d);
            return;
        }
        if (fi.content_checksum) {
            uint8_t c[4];
            if (read_exact(c, 4) != 0) { fail(-LZ4FLEX_FE_IO); return; }
            if (content_hasher.finish() != rd32(c)) { fail(-LZ4FLEX_FE_CONTENT_CHECKSUM); return; }
        }
        have_frame = false;
        pending_zero = true;
    }
    // what every decode ends with: an error surfaces after the pieces in front of it (and without a zero); else the EndMark, if that is where the gathering stopped
    void close_batch() {
        if (pending_err) pending_zero = false;
        else if (saw_end && !pending_zero) end_mark();
    }

    // One block off the stream into `comp` (frame/decompress.rs:231-278): BlockInfo word, EndMark, BlockTooBig, payload, optional
    // block checksum.  END: the EndMark (handled once the staged blocks are decoded); EOFS: no more bytes where a BlockInfo starts --
    // Ok(0), the frame stays open (:231-238; pending_zero is set); ERR: fail() was called and the payload, if any, taken back;
    // RAW / COMP: a stored / compressed block of `len` bytes at comp[at], `end` = in_total behind it.  Everything below RAW ends the gathering.
    enum BlockKind { END, EOFS, ERR, RAW, COMP };
    struct BlockRead { BlockKind kind; size_t at, len, end; };
    BlockRead read_block(size_t mbs) {
        uint8_t bi[4];
        if (read_exact(bi, 4) != 0) {
            if (io_failed) { fail(-LZ4FLEX_FE_IO); return {ERR, 0, 0, 0}; }
            pending_zero = true;
            return {EOFS, 0, 0, 0};
        }
        const uint32_t size = rd32(bi);
        if (size == 0) return {END, 0, 0, 0};
        const size_t len = size & ~BLOCK_UNCOMPRESSED_SIZE_BIT, at = comp.size();
        if (len > mbs) { fail(-LZ4FLEX_FE_BLOCK_TOO_BIG); return {ERR, 0, 0, 0}; }
        comp.resize(at + len);
        if (len && read_exact(comp.data() + at, len) != 0) { comp.resize(at); fail(-LZ4FLEX_FE_IO); return {ERR, 0, 0, 0}; }
        if (fi.block_checksums) {
            uint8_t c[4];
            if (read_exact(c, 4) != 0) { comp.resize(at); fail(-LZ4FLEX_FE_IO); return {ERR, 0, 0, 0}; }
            if (XxHash32::oneshot(0, comp.data() + at, len) != rd32(c)) { comp.resize(at); fail(-LZ4FLEX_FE_BLOCK_CHECKSUM); return {ERR, 0, 0, 0}; }
        }
        return {(size & BLOCK_UNCOMPRESSED_SIZE_BIT) ? RAW : COMP, at, len, in_total};
    }
    // Blocks off the stream for one call: at most `max_blocks`, and no more than the launch's output budget.  Compressed blocks enter the
    // launch's columns.  full_slots: every block gets a block size of output (a reader's buffer, slot i at i * block size; a Linked
    // run), else what it can decode to (decode_slot_cap; a stored block its length).  raw_ends: a stored block is the last one taken.
    void gather(size_t mbs, size_t max_blocks, bool full_slots, bool raw_ends) {
        comp.clear(); in_off.clear(); in_len.clear(); out_off.clear(); out_cap.clear(); slots.clear();
        ready.clear(); ready_idx = 0; ready_pos = 0;
        out_need = 0;
        saw_end = false;
        const size_t out_budget = launch_out_budget(batch_bytes, mbs, batch_auto);
        while (slots.size() < max_blocks && (slots.empty() || out_need + mbs <= out_budget)) {
            const BlockRead blk = read_block(mbs);
            saw_end = blk.kind == END;
            if (blk.kind < RAW) break;
            const bool raw = blk.kind == RAW;
            const size_t room = full_slots ? mbs : raw ? blk.len : decode_slot_cap(mbs, blk.len);
            slots.push_back({raw, blk.at, blk.len, blk.end, in_off.size(), out_need});
            if (!raw) { in_off.push_back(blk.at); in_len.push_back((uint32_t)blk.len); out_off.push_back(out_need); out_cap.push_back((uint32_t)room); }
            out_need += room;
            if (raw && raw_ends) break;
        }
        const size_t nb = in_off.size();
        out_len.assign(nb, 0); status.assign(nb, 0); detail.assign(2 * nb, 0);
    }

    // Independent frames: the gathered compressed blocks decoded into `sink` by one launch; false: fail() was called
    bool launch_independent(uint8_t* sink) {
        if (in_off.empty()) return true;
        const int rc = lz4flex_decompress_batch(nullptr, comp.data(), in_off.data(), in_len.data(), (uint32_t)in_off.size(), sink,
                                                out_off.data(), out_cap.data(), out_len.data(), status.data(),
                                                detail.data(), LZ4FLEX_MEM_HOST, nullptr);
        if (rc) { fail(rc); pending_zero = false; }
        return rc == 0;
    }
    // ... and a block's bytes at sink + out_at: a stored block placed, a compressed one checked; content length and hash move on.
    // false: the block failed -- the pieces before it were delivered / queued, the error surfaces after them
    bool take_slot(const Slot& s, uint8_t* sink, size_t* plen) {
        if (s.raw) memcpy(sink + s.out_at, comp.data() + s.at, s.len);
        else if (status[s.col] != 0) { fail_block(block_detail(s.col)); return false; }
        *plen = s.raw ? s.len : out_len[s.col];
        content_len += *plen;
        if (fi.content_checksum) content_hasher.write(sink + s.out_at, *plen);
        return true;
    }
    // Independent frames, staged: up to a batch of blocks decoded into `out` by one launch; every block is a piece of the ready list
    void decode_independent() {
        const size_t mbs = block_size_bytes(fi.block_size);
        ready_linked = false;
        gather(mbs, blocks_per_launch(batch_bytes, mbs, batch_auto), false, false);
        if (out.size() < out_need) out.resize(out_need);
        size_t plen;
        if (launch_independent(out.data()))
            for (const Slot& s : slots) {
                if (!take_slot(s, out.data(), &plen)) break;
                ready.push_back({s.out_at, plen, s.end});
            }
        close_batch();
    }
    // Independent frames, direct (round 6): the reader asked for at least a block's worth of bytes (lz4flex_frame_decompress: for all of
    // them) -- the blocks are decoded STRAIGHT INTO ITS BUFFER, slot i at i * block size, and the number of bytes delivered is returned
    // (0: nothing went that way, the ready list says what there is).  Staging them and copying them out was a host copy of every decoded
    // byte: 12 instead of ~ 20 GiB/s through host buffers.  A slot that is not full (a flush() boundary, the frame's last block) is closed
    // up by moving what follows it; a block that decodes to nothing -- after which read() returns 0 once, frame/decompress.rs:344-349 --
    // and everything behind it goes to the staging buffer as pieces of the ready list.
    size_t decode_independent_direct(uint8_t* buf, size_t len) {
        const size_t mbs = block_size_bytes(fi.block_size);
        ready_linked = false;
        gather(mbs, std::min(blocks_per_launch(batch_bytes, mbs, batch_auto), len / mbs), true, false);
        size_t delivered = 0, staged_at = 0, plen;
        bool staged = false;           // a block decoded to nothing: from there on the pieces wait in `out`
        if (launch_independent(buf))
            for (const Slot& s : slots) {
                if (!take_slot(s, buf, &plen)) break;
                if (!staged && plen == 0) {
                    staged = true;
                    if (out.size() < out_need) out.resize(out_need);
                }
                if (!staged) {
                    if (s.out_at != delivered && plen) memmove(buf + delivered, buf + s.out_at, plen);
                    delivered += plen;
                } else {
                    if (plen) memcpy(out.data() + staged_at, buf + s.out_at, plen);
                    ready.push_back({staged_at, plen, s.end});
                    staged_at += plen;
                }
            }
        close_batch();
        return delivered;
    }

    // Linked frames (frame/decompress.rs:195-222,280-306: the reference decodes block after block into one window, a block's
    // matches may reach up to 64 KiB behind its start).  Here a run of compressed blocks is decoded by ONE launch
    // (LZ4FLEX_MEM_CHAINED): the staging buffer `ldst` holds [the frame's last <= 64 KiB | block | block | ...], block k is
    // given the position behind its predecessors as its initial sink position and the kernel makes it wait for them only where
    // a match really reaches behind its start -- the blocks of a frame written by this library's throughput encoder never do.
    // A block's decoded size is not in the frame: every block but a frame's last is taken to fill the block size, and the
    // blocks behind one that did not (a flush() boundary, frame/compress.rs:398-403) are decoded again from their real position
    // (DecodeRuns).  A block stored raw ends a run (its bytes are placed by the host).
    // What one call produces behind the `carry` bytes of history at the front of ldst: `produced` bytes, handed out where they are as
    // one piece, cut where a block decoded to nothing -- there a read returns 0 once (read_more() == 0, frame/decompress.rs:344-349)
    // with the bytes in front of it delivered and the ones behind it still to come.  piece_at: where the piece being made starts.
    struct LinkedOut { size_t carry, produced, piece_at; };
    void end_piece(LinkedOut& o, size_t src_end) {
        if (o.produced != o.piece_at) ready.push_back({o.carry + o.piece_at, o.produced - o.piece_at, src_end});
        o.piece_at = o.produced;
    }
    void empty_block(LinkedOut& o, size_t src_end) {
        end_piece(o, src_end);
        ready.push_back({o.carry + o.produced, 0, src_end});
    }
    void grow_ldst(size_t n) { if (ldst.size() < n) ldst.resize(n); }
    // the run of `nb` compressed blocks: launches until every block sits behind its real predecessor; false: a launch or a block failed
    // (fail() was called; what was decoded in front of it is still handed out)
    bool decode_run(size_t mbs, size_t nb, LinkedOut& o) {
        std::vector<uint32_t> pos(nb), cap(nb);
        std::vector<uint64_t> zero_off(nb, 0);
        DecodeRuns runs(nb);
        for (size_t first = 0; first < nb;) {
            const size_t m = runs.take(first), room = runs.first_room(first, mbs, ring);
            grow_ldst(o.carry + o.produced + (m - 1) * mbs + room);
            for (size_t k = 0; k < m; k++) {
                pos[k] = (uint32_t)(o.carry + o.produced + k * mbs);
                cap[k] = pos[k] + (uint32_t)(k == 0 ? room : mbs);
            }
            lz4flex_decompress_ext ext{}; ext.out_pos = pos.data();
            const int rc = lz4flex_decompress_batch_ex(nullptr, comp.data(), in_off.data() + first, in_len.data() + first, (uint32_t)m,
                                                       ldst.data(), zero_off.data(), cap.data(), out_len.data() + first, status.data() + first,
                                                       detail.data() + 2 * first, &ext, LZ4FLEX_MEM_HOST | LZ4FLEX_MEM_CHAINED, nullptr);
            if (rc) { fail(rc); pending_zero = false; return false; }
            size_t k = 0;          // blocks of this launch that were accepted
            bool retry = false, failed = false;
            for (; k < m; k++) {
                const size_t i = first + k;
                if (!runs.is_roomy(i)) ring.enter(mbs);       // (once per block: the roomy block entered when it was first tried)
                if (status[i] != 0) {
                    retry = status[i] == LZ4FLEX_E_OUTPUT_TOO_SMALL && !runs.is_roomy(i) && ring.room(mbs) > mbs;
                    if (!retry) {
                        lz4flex_err_detail d = block_detail(i);
                        if (status[i] == LZ4FLEX_E_OUTPUT_TOO_SMALL) ring.too_small(mbs, pos[k], &d.expected, &d.actual);
                        fail_block(d);
                        failed = true;
                    }
                    break;
                }
                o.produced += out_len[i];
                ring.advance(out_len[i]);
                if (out_len[i] == 0) empty_block(o, slots[i].end);
                if (out_len[i] != mbs) { k++; break; }        // the blocks behind a short one were given a wrong position
            }
            if (failed) return false;
            runs.ended(first, m, k, retry);
            first += k;
        }
        return true;
    }
    // a block stored raw behind the run
    void place_raw(size_t mbs, const Slot& s, LinkedOut& o) {
        grow_ldst(o.carry + o.produced + s.len);
        memcpy(ldst.data() + o.carry + o.produced, comp.data() + s.at, s.len);
        o.produced += s.len;
        ring.enter(mbs);
        ring.advance(s.len);
        if (s.len == 0) empty_block(o, s.end);
    }
    void decode_linked() {
        const size_t mbs = block_size_bytes(fi.block_size);
        ready_linked = true;
        // The previous call's bytes were handed out straight from ldst (no copy), so its last 64 KiB are moved to the front only now that
        // they have been consumed.
        if (lhave > WINDOW_SIZE) {
            memmove(ldst.data(), ldst.data() + (lhave - WINDOW_SIZE), WINDOW_SIZE);
            lhave = WINDOW_SIZE;
        }
        LinkedOut o{lhave, 0, 0};
        // 1. gather: a run of compressed blocks, and the stored block that ended it
        gather(mbs, std::min(blocks_per_launch(batch_bytes, mbs, batch_auto), pos_blocks(o.carry, mbs)), true, true);
        const size_t nb = in_off.size();
        grow_ldst(o.carry + (nb + 1) * mbs);
        // 2. decode the run; 3. place a raw tail
        if (decode_run(mbs, nb, o) && slots.size() > nb) place_raw(mbs, slots[nb], o);
        // 4. hand the bytes out where they are (ready items index `ldst` in Linked mode); they stay there as history
        end_piece(o, 0);
        content_len += o.produced;
        if (fi.content_checksum && o.produced) content_hasher.write(ldst.data() + o.carry, o.produced);
        lhave = o.carry + o.produced;
        close_batch();
    }

    // What read and fill_buf share (frame/decompress.rs:353-367, :410-416), in this order: the ready pieces, the pending error, the
    // pending zero, the next frame's header, more blocks.  PIECE: ready[ready_idx] holds bytes for the caller to take; else the value to
    // return -- 0 behind an empty block (read_more() == 0), at the end of a frame and at EOF, -code, or (`direct`, a reader's buffer
    // of at least a block and DIRECT_MIN bytes, Independent frames) the number of bytes decoded straight into it.
    static constexpr int64_t PIECE = INT64_MIN;
    int64_t next_piece(lz4flex_err_detail* d, uint8_t* direct = nullptr, size_t direct_len = 0) {
        for (;;) {
            if (ready_idx < ready.size()) {
                const Item& it = ready[ready_idx];
                if (it.len != 0) return PIECE;
                zero_end = it.src_end; ready_idx++; ready_pos = 0;
                return 0;
            }
            if (pending_err) { if (d) *d = pending_detail; return pending_err; }
            if (pending_zero) { pending_zero = false; return 0; }
            if (!have_frame) {
                lz4flex_err_detail hd{};
                const int rc = read_frame_info(&hd);
                if (rc == 1) return 0;
                if (rc < 0) { if (d) *d = hd; return rc; }
            }
            if (fi.block_mode == 1) decode_linked();
            else if (direct && direct_len >= block_size_bytes(fi.block_size) && direct_len >= DIRECT_MIN) {
                const size_t n = decode_independent_direct(direct, direct_len);
                if (n) return (int64_t)n;
            } else decode_independent();
        }
    }
    void took(size_t n) {
        ready_pos += n;
        if (ready_pos == ready[ready_idx].len) { ready_idx++; ready_pos = 0; }
    }
    // io::BufRead::fill_buf, frame/decompress.rs:410-416: the decoded bytes not consumed yet (decodes more when there are
    // none); *p stays valid until the next call on this decoder.  0 = end of frame / EOF (an empty slice), < 0 = -code.
    int64_t fill_buf(const uint8_t** p, lz4flex_err_detail* d) {
        const int64_t rc = next_piece(d);
        if (rc == 0) *p = out.data();
        if (rc != PIECE) return rc;
        const Item& it = ready[ready_idx];
        *p = ready_base() + it.off + ready_pos;
        return (int64_t)(it.len - ready_pos);
    }
    // io::BufRead::consume, :418-421 (the reference asserts amt <= available)
    int consume(size_t amt) {
        if (amt == 0) return 0;
        if (ready_idx >= ready.size() || amt > ready[ready_idx].len - ready_pos) return -LZ4FLEX_E_INVALID_ARG;
        took(amt);
        return 0;
    }
    // io::Read::read, frame/decompress.rs:353-367
    int64_t read(uint8_t* buf, size_t len, lz4flex_err_detail* d) {
        const int64_t rc = next_piece(d, buf, len);
        if (rc != PIECE) return rc;
        const Item& it = ready[ready_idx];
        const size_t n = std::min(it.len - ready_pos, len);
        if (n == 0) return 0;   // zero-length destination
        memcpy(buf, ready_base() + it.off + ready_pos, n);
        took(n);
        return (int64_t)n;
    }
};

extern "C" {

lz4flex_frame_encoder* lz4flex_frame_encoder_new(const lz4flex_frame_info* info, lz4flex_write_fn w, void* user) {
    if (!w) return nullptr;
    lz4flex_frame_encoder* e = new (std::nothrow) lz4flex_frame_encoder();
    if (!e) return nullptr;
    if (info) e->fi = *info;
    e->w = w; e->user = user;
    return e;
}
int64_t lz4flex_frame_encoder_write(lz4flex_frame_encoder* e, const uint8_t* buf, size_t len) {
    if (!e || (!buf && len)) return -LZ4FLEX_E_INVALID_ARG;
    return e->write(buf, len);
}
int lz4flex_frame_encoder_flush(lz4flex_frame_encoder* e) { return e ? e->flush() : -LZ4FLEX_E_INVALID_ARG; }
int lz4flex_frame_encoder_try_finish(lz4flex_frame_encoder* e, lz4flex_err_detail* d) {
    if (d) memset(d, 0, sizeof *d);
    return e ? e->try_finish(d) : -LZ4FLEX_E_INVALID_ARG;
}
void lz4flex_frame_encoder_frame_info(lz4flex_frame_encoder* e, lz4flex_frame_info* out) { if (e && out) *out = e->fi; }
int lz4flex_frame_encoder_set_batch_bytes(lz4flex_frame_encoder* e, size_t bytes) {
    if (!e || e->is_frame_open || bytes == 0) return -LZ4FLEX_E_INVALID_ARG;
    e->batch_bytes = bytes;
    e->batch_auto = false;
    return 0;
}
void lz4flex_frame_encoder_free(lz4flex_frame_encoder* e) { delete e; }

lz4flex_frame_decoder* lz4flex_frame_decoder_new(lz4flex_read_fn r, void* user) {
    if (!r) return nullptr;
    lz4flex_frame_decoder* d = new (std::nothrow) lz4flex_frame_decoder();
    if (!d) return nullptr;
    d->r = r; d->user = user;
    return d;
}
int64_t lz4flex_frame_decoder_read(lz4flex_frame_decoder* dcd, uint8_t* buf, size_t len, lz4flex_err_detail* d) {
    if (!dcd || (!buf && len)) return -LZ4FLEX_E_INVALID_ARG;
    if (d) memset(d, 0, sizeof *d);
    return dcd->read(buf, len, d);
}
int64_t lz4flex_frame_decoder_fill_buf(lz4flex_frame_decoder* dcd, const uint8_t** buf, lz4flex_err_detail* d) {
    if (!dcd || !buf) return -LZ4FLEX_E_INVALID_ARG;
    if (d) memset(d, 0, sizeof *d);
    return dcd->fill_buf(buf, d);
}
int lz4flex_frame_decoder_consume(lz4flex_frame_decoder* dcd, size_t amt) {
    if (!dcd) return -LZ4FLEX_E_INVALID_ARG;
    return dcd->consume(amt);
}
int lz4flex_frame_decoder_set_batch_bytes(lz4flex_frame_decoder* d, size_t bytes) {
    if (!d || bytes == 0) return -LZ4FLEX_E_INVALID_ARG;
    d->batch_bytes = bytes;
    d->batch_auto = false;
    return 0;
}
void lz4flex_frame_decoder_free(lz4flex_frame_decoder* d) { delete d; }

// ---- one-shot helpers over flat buffers -------------------------------------------------------
namespace {
struct FlatW { uint8_t* p; size_t pos, cap; bool full; };
int64_t flat_write(void* u, const uint8_t* b, size_t n) {
    FlatW* f = (FlatW*)u;
    if (f->cap - f->pos < n) { f->full = true; return -1; }
    memcpy(f->p + f->pos, b, n); f->pos += n;
    return (int64_t)n;
}
struct FlatR { const uint8_t* p; size_t pos, len; };
int64_t flat_read(void* u, uint8_t* b, size_t n) {
    FlatR* f = (FlatR*)u;
    const size_t k = std::min(n, f->len - f->pos);
    memcpy(b, f->p + f->pos, k); f->pos += k;
    return (int64_t)k;
}
}  // namespace

size_t lz4flex_frame_compress_bound(size_t in_len, const lz4flex_frame_info* info) {
    int bs = info ? info->block_size : 0;
    if (bs == 0) bs = block_size_from_buf_length(in_len);
    const size_t mbs = block_size_bytes(bs) ? block_size_bytes(bs) : 65536;
    const size_t nblk = (in_len + mbs - 1) / mbs;
    return MAX_FRAME_INFO_SIZE + in_len + nblk * 8 + 8;   // raw-stored worst case: 4 B header (+4 B checksum) per block
}

int64_t lz4flex_frame_compress(const uint8_t* in, size_t in_len, const lz4flex_frame_info* info, uint8_t* out,
                               size_t out_cap, lz4flex_err_detail* detail) {
    if ((!in && in_len) || !out) return -LZ4FLEX_E_INVALID_ARG;
    if (detail) memset(detail, 0, sizeof *detail);
    FlatW fw{out, 0, out_cap, false};
    lz4flex_frame_encoder* e = lz4flex_frame_encoder_new(info, flat_write, &fw);
    if (!e) return -LZ4FLEX_E_NOMEM;
    e->final_write = true;                     // (whole blocks AND the remainder are compressed where they lie: no staging copy)
    int64_t rc = e->write(in, in_len);
    if (rc >= 0) rc = e->try_finish(detail);
    lz4flex_frame_encoder_free(e);
    if (rc < 0) return fw.full ? -LZ4FLEX_FE_OUTPUT_FULL : rc;
    return (int64_t)fw.pos;
}

int64_t lz4flex_frame_decompress(const uint8_t* in, size_t in_len, uint8_t* out, size_t out_cap, size_t* consumed,
                                 lz4flex_err_detail* detail) {
    if ((!in && in_len) || (!out && out_cap)) return -LZ4FLEX_E_INVALID_ARG;
    if (detail) memset(detail, 0, sizeof *detail);
    FlatR fr{in, 0, in_len};
    lz4flex_frame_decoder* d = lz4flex_frame_decoder_new(flat_read, &fr);
    if (!d) return -LZ4FLEX_E_NOMEM;
    size_t pos = 0;
    int64_t rc = 0;
    uint8_t scratch[1];
    for (;;) {   // read_to_end: until read() returns 0
        if (pos == out_cap) {
            // probe for more data without a destination
            rc = d->read(scratch, 1, detail);
            if (rc > 0) rc = -LZ4FLEX_FE_OUTPUT_FULL;
            break;
        }
        rc = d->read(out + pos, out_cap - pos, detail);
        if (rc <= 0) break;
        pos += (size_t)rc;
    }
    // (the decoder gathers blocks ahead of the one it hands out: where an empty block ended the reading, the reference's reader stands behind
    // that block, frame/decompress.rs:344-349,392-407)
    if (consumed) *consumed = rc == 0 && d->zero_end != (size_t)-1 ? d->zero_end : fr.pos;
    lz4flex_frame_decoder_free(d);
    return rc < 0 ? rc : (int64_t)pos;
}

}  // extern "C"
