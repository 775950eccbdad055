// lz4_batch_entry.h -- lz4flex_compress_batch as the frame layer calls it (frame.cpp, frame_many.cpp; defined in capi.cpp).  Internal: not
// an lz4flex_* export, not installed.  No HIP include: frame.cpp is plain host code.
#pragma once
#include <stdint.h>

struct lz4flex_ctx;

namespace lz4flex_dev {
// lz4flex_compress_batch's arguments, checks and results; linked_frame = the blocks are a Linked frame's, their LZ4FLEX_BLOCK_HISTORY
// bits the stream in front of them -- the one thing about such a call that encode_route (lz4_route.h) cannot see in the arrays.  The
// public entry is this with linked_frame false.  No setting is written: a context other threads share is left as it is.
int compress_batch_entry(lz4flex_ctx* ctx, const void* in_base, const uint64_t* in_off, const uint32_t* in_len, const uint32_t* flags, uint32_t n,
                         void* out_base, const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len, int32_t* status, int mem_kind,
                         void* hip_stream, bool linked_frame);
}  // namespace lz4flex_dev
