// frame_plan_shim.cpp -- C entry points over lz4_flex_amd/csrc/frame_plan.h for tests/test_frame_plan.py (ctypes).  Test infrastructure.
#include "../../lz4_flex_amd/csrc/frame_plan.h"

using namespace lz4flex_plan;

extern "C" {

uint64_t fp_block_size_bytes(int code) { return block_size_bytes(code); }
int fp_block_size_from_buf_length(uint64_t n) { return block_size_from_buf_length(n); }
uint64_t fp_stream_max() { return STREAM_MAX; }
uint64_t fp_window_size() { return WINDOW_SIZE; }
uint32_t fp_uncompressed_bit() { return BLOCK_UNCOMPRESSED_SIZE_BIT; }

// modes[skip + i] .. of a TableOffset that first takes `skip` full blocks (what sharded.cpp replays), then lens[0 .. n)
void fp_table_modes(uint64_t mbs, uint64_t skip, const uint64_t* lens, uint64_t n, uint32_t* modes) {
    TableOffset t;
    for (uint64_t k = 0; k < skip; k++) (void)t.next(mbs, mbs);
    for (uint64_t i = 0; i < n; i++) modes[i] = t.next(mbs, lens[i]);
}

// a LinkedWindow reset to `pos` walks lens[0 .. n): out[8 i ..] = in_off, dict_off, in_len, in_pos, dict_len, so, repos, flags;
// keep[i] = keep_from() behind block i
void fp_linked_walk(uint64_t mbs, uint64_t pos, const uint64_t* lens, uint64_t n, uint64_t* out, uint64_t* keep) {
    LinkedWindow w;
    w.reset(pos);
    for (uint64_t i = 0; i < n; i++) {
        const lz4flex_chain_block b = w.next(mbs, lens[i]);
        uint64_t* o = out + 8 * i;
        o[0] = b.in_off; o[1] = b.dict_off; o[2] = b.in_len; o[3] = b.in_pos; o[4] = b.dict_len; o[5] = b.so; o[6] = b.repos; o[7] = b.flags;
        keep[i] = w.keep_from();
    }
}

}  // extern "C"
