// frame_plan.h -- what a FrameEncoder decides about a block from the lengths of the blocks before it (reference
// src/frame/header.rs, src/frame/compress.rs:261-371), stated once for frame.cpp (the streaming encoder), frame_many.cpp (N frames per
// launch) and sharded.cpp (one frame across ranks); and what frame.cpp's FrameDecoder decides about a Linked frame's block from the
// decoded lengths of the blocks before it (src/frame/decompress.rs:195-222, :280-306): DecodeRing, DecodeRuns.  Pure integer functions: host
// only, no HIP, no kernel includes it; tests/test_frame_plan.py walks them on a CPU, past the table reposition near 2 GiB that no test
// reaches through the API and through ring wraps and relaunches that only a frame of the right shape reaches on the GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/lz4flex_amd.h"

namespace lz4flex_plan {

constexpr uint32_t BLOCK_UNCOMPRESSED_SIZE_BIT = 0x80000000u;   // BlockInfo: the payload is the block itself (header.rs:32)
constexpr uint64_t WINDOW_SIZE = 64 * 1024;                     // how far back a match reaches
constexpr uint64_t FAST_HISTORY = 32768;                        // throughput encoder, Linked frame: bytes of the stream in front of a block that are its history
constexpr uint64_t REPOSITION_AT = 0xFFFFFFFFu / 2;             // compress.rs:266: a table offset that could reach this is taken back first
// A stream of at most this many bytes never repositions, whatever its block size and mode (tests/test_frame_plan.py walks exactly
// this length): frame_many.cpp lays out all blocks of such a stream for one launch and sends longer ones through the one-shot call.
constexpr uint64_t STREAM_MAX = 0x7FFF0000ull - (8u << 20);

// BlockSize::get_size, header.rs:68-77
inline size_t block_size_bytes(int code) {
    switch (code) {
        case 4: return 64u * 1024;
        case 5: return 256u * 1024;
        case 6: return 1024u * 1024;
        case 7: return 4u * 1024 * 1024;
        case 8: return 8u * 1024 * 1024;
        default: return 0;
    }
}
// BlockSize::from_buf_length, header.rs:57-67
inline int block_size_from_buf_length(uint64_t n) { return n > 256u * 1024 ? 7 : (n > 64u * 1024 ? 5 : 4); }

// Independent frame: the table mode of the next block, `len` bytes of a frame of `mbs`-byte blocks (compress.rs:266-271, :357-367).
// The table is as good as new where the stream offset is 0: block 0, and the first block after each reposition.
struct TableOffset {
    uint64_t so = 0;              // src_stream_offset
    uint32_t next(size_t mbs, size_t len) {
        if (so + mbs + WINDOW_SIZE >= REPOSITION_AT) so = 0;
        const uint32_t mode = so == 0 ? LZ4FLEX_BLOCK_FRAME_FIRST : LZ4FLEX_BLOCK_FRAME_CONTINUATION;
        so += len;
        return mode;
    }
};

// Linked frame: the reference's src ring (prefix + ext_dict, compress.rs:62-93, :324-356) in coordinates of the stream.
struct LinkedWindow {
    uint64_t vbase = 0;               // stream position of the reference's src[0]
    uint64_t v_src_start = 0;         // == src_start == src_end between blocks
    uint64_t dict_stream = 0;         // stream position of ext_dict[0]
    uint64_t src_stream_offset = 0;
    uint32_t ext_dict_len = 0;
    // a new frame whose first byte is the stream's byte `pos`
    void reset(uint64_t pos) { *this = LinkedWindow(); vbase = pos; }
    // the first stream byte the blocks to come can still reach
    uint64_t keep_from() const { return ext_dict_len ? std::min(vbase, dict_stream) : vbase; }
    // the next block of `len` bytes: its compress_internal arguments with in_off / dict_off as stream positions
    lz4flex_chain_block next(size_t mbs, size_t len) {
        lz4flex_chain_block b{};
        if (src_stream_offset + mbs + WINDOW_SIZE >= REPOSITION_AT) {                    // :266-271
            b.repos = (uint32_t)(src_stream_offset - ext_dict_len);
            src_stream_offset = ext_dict_len;
        }
        const uint64_t v_src_end = v_src_start + len;
        b.in_off = vbase;
        b.in_len = (uint32_t)v_src_end;
        b.in_pos = (uint32_t)v_src_start;
        b.dict_off = ext_dict_len ? dict_stream : 0;
        b.dict_len = ext_dict_len;
        b.so = (uint32_t)src_stream_offset;
        v_src_start = v_src_end;                                                         // :324-356 buffer / offset maintenance
        if (v_src_start >= mbs + WINDOW_SIZE) {
            dict_stream = vbase + v_src_end - WINDOW_SIZE;
            ext_dict_len = (uint32_t)WINDOW_SIZE;
            src_stream_offset += v_src_end;
            vbase += v_src_end;
            v_src_start = 0;
        } else if (v_src_start + ext_dict_len > WINDOW_SIZE) {
            const uint64_t delta = std::min<uint64_t>(ext_dict_len, v_src_start + ext_dict_len - WINDOW_SIZE);
            dict_stream += delta;
            ext_dict_len -= (uint32_t)delta;
        }
        return b;
    }
};

// ---- how a launch is sized (frame.cpp; the slot stride also sharded.cpp)
// Blocks gathered per kernel launch.  A block is one serial chain on the device (a 4 MiB block takes 64x as long as a 64 KiB one), so
// throughput needs MANY blocks in flight: by default at least 256 blocks per launch (one per CU), capped at 1 GiB of staged input; an
// explicit set_batch_bytes is honoured exactly.
inline size_t blocks_per_launch(size_t batch_bytes, size_t mbs, bool automatic) {
    size_t nb = std::max<size_t>(1, batch_bytes / mbs);
    if (automatic) nb = std::max<size_t>(nb, std::min<size_t>(256, ((size_t)1 << 30) / mbs));
    return nb;
}
// encoder: the distance between the compressed slots of a launch
inline size_t slot_stride(size_t mbs) { return (lz4flex_get_maximum_output_size(mbs) + 63) / 64 * 64; }
// decoder: the sink of a compressed block of `len` bytes.  An LZ4 block expands by less than 255x (one length byte adds at most 255
// output bytes), so this is as good a sink as the reference's block-size buffer and a frame of tiny blocks cannot make the read-ahead
// reserve (and the device arena mirror) gigabytes.
inline size_t decode_slot_cap(size_t mbs, size_t len) { return std::min<size_t>(mbs, 255u * len + 64u); }
// decoder: bytes of output reserved per launch
inline size_t launch_out_budget(size_t batch_bytes, size_t mbs, bool automatic) { return std::max(batch_bytes, mbs) * (automatic ? 4u : 1u); }
// Linked decoder: blocks per launch behind `carry` bytes of history.  Sink positions are 32-bit: an explicit batch size of 4 GiB or
// more must not wrap them; halved, since a block may be given up to two block sizes of room (DecodeRing::sink_end).
inline size_t pos_blocks(size_t carry, size_t mbs) { return ((size_t)((0xFFFFFFFFull - carry) / mbs) - 1u) / 2u; }

// Linked frame, decoding: the reference's dst ring of 2 block sizes + 64 KiB (frame/decompress.rs:62-72, :145-156) on lengths alone,
// for the two things it decides: the sink of a compressed block -- a block size behind ring_start (the reference's dst_start); once
// the ring has wrapped, everything up to the external dictionary's start, as much as TWO block sizes -- and the positions an
// OutputTooSmall names.
struct DecodeRing {
    size_t ext_dict_offset = 0, ext_dict_len = 0, ring_start = 0;
    void reset() { *this = DecodeRing(); }
    // before every block (:195-222): wrap where a block no longer fits behind ring_start; else shrink the dictionary to the window
    void enter(size_t mbs) {
        if (ring_start + mbs > 2 * mbs + WINDOW_SIZE) { ext_dict_offset = ring_start - WINDOW_SIZE; ext_dict_len = WINDOW_SIZE; ring_start = 0; }
        else if (ring_start + ext_dict_len > WINDOW_SIZE) {
            const size_t delta = std::min<size_t>(ext_dict_len, ring_start + ext_dict_len - WINDOW_SIZE);
            ext_dict_offset += delta; ext_dict_len -= delta;
        }
    }
    size_t sink_end(size_t mbs) const { return ext_dict_len ? ext_dict_offset : ring_start + mbs; }   // :280-306
    size_t room(size_t mbs) const { return sink_end(mbs) - ring_start; }
    void advance(size_t n) { ring_start += n; }                                                       // :356-360, :418-421: the reader took the block
    // a kernel's OutputTooSmall (expected, actual) of a block whose sink started at `pos`, as the reference's sink has them (:288-305)
    void too_small(size_t mbs, uint64_t pos, uint64_t* expected, uint64_t* actual) const { *expected = *expected - pos + ring_start; *actual = sink_end(mbs); }
};

// Linked frame, decoding a run of `nb` compressed blocks: one launch gives every block a sink of one block size and takes every block
// but a frame's last to fill it; the blocks behind one that did not (a flush() boundary) were given a wrong position and are decoded
// again.  If every launch took the whole rest of the run, a frame of many short blocks would cost a launch and a re-decode of everything
// behind it per block: the run length is cut to a quarter whenever a launch stops early and doubles while launches end clean, so launches
// and decoded blocks stay linear in the number of blocks.  A block that ran out of room where the reference's sink is larger (right
// behind a wrap of its ring) comes back once, alone, with that room: the roomy block.
struct DecodeRuns {
    size_t nb, run, roomy = (size_t)-1;
    explicit DecodeRuns(size_t blocks) : nb(blocks), run(blocks) {}
    bool is_roomy(size_t i) const { return i == roomy; }
    size_t take(size_t first) const { return is_roomy(first) ? 1 : std::min(run, nb - first); }      // blocks of the launch that starts at `first`
    size_t first_room(size_t first, size_t mbs, const DecodeRing& r) const { return is_roomy(first) ? r.room(mbs) : mbs; }
    // the launch of `m` blocks at `first` accepted `k` of them; retry: block first + k comes back as the roomy one (`run` stays)
    void ended(size_t first, size_t m, size_t k, bool retry) {
        if (retry) roomy = first + k;
        else run = k < m ? std::max<size_t>(1, m / 4) : std::min(nb, 2 * m);
    }
};

}  // namespace lz4flex_plan
