// frame_plan.h -- what a FrameEncoder decides about a block from the lengths of the blocks before it (reference
// src/frame/header.rs, src/frame/compress.rs:261-371), stated once for frame.cpp (the streaming encoder), frame_many.cpp (N frames per
// launch) and sharded.cpp (one frame across ranks).  Pure integer functions: host only, no HIP, no kernel includes it;
// tests/test_frame_plan.py walks them on a CPU, past the table reposition near 2 GiB that no test reaches through the API.
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

}  // namespace lz4flex_plan
