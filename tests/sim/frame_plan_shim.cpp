// frame_plan_shim.cpp -- C entry points over lz4_flex_amd/csrc/frame_plan.h for tests/test_frame_plan.py (ctypes).  Test infrastructure.
// With -DFRAME_PLAN_SHIM_MAIN: a stand-alone program over the decoder's entries (sanitizer builds).
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

uint64_t fp_blocks_per_launch(uint64_t batch_bytes, uint64_t mbs, int automatic) { return blocks_per_launch(batch_bytes, mbs, automatic != 0); }
uint64_t fp_decode_slot_cap(uint64_t mbs, uint64_t len) { return decode_slot_cap(mbs, len); }
uint64_t fp_launch_out_budget(uint64_t batch_bytes, uint64_t mbs, int automatic) { return launch_out_budget(batch_bytes, mbs, automatic != 0); }
uint64_t fp_pos_blocks(uint64_t carry, uint64_t mbs) { return pos_blocks(carry, mbs); }

// a DecodeRing walks blocks that decode to lens[0 .. n) bytes: out[5 i ..] = sink_end, ext_dict_offset, ext_dict_len, ring_start, room as
// block i finds them behind enter(); then advance(lens[i])
void fp_decode_ring_walk(uint64_t mbs, const uint64_t* lens, uint64_t n, uint64_t* out) {
    DecodeRing r;
    r.ext_dict_offset = 7; r.ext_dict_len = 9; r.ring_start = 11;      // (reset() has to clear them)
    r.reset();
    for (uint64_t i = 0; i < n; i++) {
        r.enter(mbs);
        uint64_t* o = out + 5 * i;
        o[0] = r.sink_end(mbs); o[1] = r.ext_dict_offset; o[2] = r.ext_dict_len; o[3] = r.ring_start; o[4] = r.room(mbs);
        r.advance(lens[i]);
    }
}

// a ring in the given state translates a kernel's OutputTooSmall (expected, actual) of a block whose sink started at `pos`
void fp_decode_ring_too_small(uint64_t mbs, uint64_t ext_dict_offset, uint64_t ext_dict_len, uint64_t ring_start, uint64_t pos,
                              uint64_t expected, uint64_t actual, uint64_t* out) {
    DecodeRing r;
    r.ext_dict_offset = ext_dict_offset; r.ext_dict_len = ext_dict_len; r.ring_start = ring_start;
    r.too_small(mbs, pos, &expected, &actual);
    out[0] = expected; out[1] = actual;
}

// DecodeRuns over nb blocks, driven as frame.cpp drives it.  kind[i]: 0 a block that fills the block size, 1 a short one (it is accepted, the
// launch stops behind it), 2 one that asks for the ring's room when first tried (and fills the block size when it comes back alone).
// out[3 j ..] = first, blocks, room of the first block of launch j (the ring: wrapped, twice `mbs` of room); returns the launches
uint64_t fp_decode_runs(uint64_t mbs, const uint8_t* kind, uint64_t nb, uint64_t* out, uint64_t max_launches) {
    DecodeRing ring;
    ring.ext_dict_offset = 2 * mbs; ring.ext_dict_len = WINDOW_SIZE;
    DecodeRuns runs(nb);
    uint64_t launches = 0;
    for (size_t first = 0; first < nb && launches < max_launches; launches++) {
        const size_t m = runs.take(first);
        out[3 * launches] = first; out[3 * launches + 1] = m; out[3 * launches + 2] = runs.first_room(first, mbs, ring);
        size_t k = 0;
        bool retry = false;
        for (; k < m; k++) {
            const size_t i = first + k;
            if (kind[i] == 2 && !runs.is_roomy(i)) { retry = true; break; }
            if (kind[i] == 1) { k++; break; }
        }
        runs.ended(first, m, k, retry);
        first += k;
    }
    return launches;
}

}  // extern "C"

#ifdef FRAME_PLAN_SHIM_MAIN
// the same entries as a stand-alone program (sanitizer builds): every block size, a ring that wraps many times, runs of every kind
#include <cstdio>
#include <vector>
int main() {
    for (int code = 4; code <= 7; code++) {
        const uint64_t mbs = block_size_bytes(code), n = 4000;
        std::vector<uint64_t> lens(n), ring(5 * n), runs(3 * n);
        std::vector<uint8_t> kind(n);
        uint64_t x = 88172645463325252ull + (uint64_t)code, wraps = 0;
        for (uint64_t i = 0; i < n; i++) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            lens[i] = x % 5 == 0 ? x % (mbs + 1) : x % 7 == 0 ? 0 : mbs;
            kind[i] = lens[i] != mbs ? 1 : x % 11 == 0 ? 2 : 0;
        }
        fp_decode_ring_walk(mbs, lens.data(), n, ring.data());
        for (uint64_t i = 0; i < n; i++) {
            if (ring[5 * i + 4] < mbs || ring[5 * i + 4] > 2 * mbs) { printf("block %llu: room %llu\n", (unsigned long long)i, (unsigned long long)ring[5 * i + 4]); return 1; }
            wraps += i > 0 && ring[5 * i + 3] == 0;
        }
        const uint64_t launches = fp_decode_runs(mbs, kind.data(), n, runs.data(), n);
        uint64_t decoded = 0;
        for (uint64_t j = 0; j < launches; j++) decoded += runs[3 * j + 1];
        if (wraps < 100 || launches == n || decoded > 8 * n) { printf("size %d: %llu wraps, %llu launches, %llu decoded\n", code, (unsigned long long)wraps, (unsigned long long)launches, (unsigned long long)decoded); return 1; }
        uint64_t two[2];
        fp_decode_ring_too_small(mbs, 2 * mbs, WINDOW_SIZE, 100, 70000, 70000 + mbs + 1, 70000 + mbs, two);
        if (two[0] != 100 + mbs + 1 || two[1] != 2 * mbs) return 1;
        (void)fp_blocks_per_launch(64u << 20, mbs, 1); (void)fp_decode_slot_cap(mbs, 0); (void)fp_launch_out_budget(1, mbs, 0); (void)fp_pos_blocks(65536, mbs);
    }
    printf("frame_plan_shim: ok\n");
    return 0;
}
#endif
