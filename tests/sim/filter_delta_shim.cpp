// Host build of the lane-local helpers of the delta filter stage (lz4_flex_amd/csrc/lz4_filter_delta.h), for tests/test_delta_filter_model.py:
// the functions the kernels of lz4_filter.hip call on a lane's 16 elements, compiled by g++ as they are.
#include <stdint.h>

#include "../../lz4_flex_amd/csrc/lz4_filter_delta.h"

namespace d = lz4flex_delta;

extern "C" {

// w: 4 E dwords (16 elements), in place.  Returns 0, or -1 for an E that is none of 1, 2, 4, 8.
int fd_delta16(int E, uint32_t* w, uint64_t prev, uint32_t ri) {
    switch (E) {
        case 1: d::delta16<1>(w, prev, ri); return 0;
        case 2: d::delta16<2>(w, prev, ri); return 0;
        case 4: d::delta16<4>(w, prev, ri); return 0;
        case 8: d::delta16<8>(w, prev, ri); return 0;
        default: return -1;
    }
}

// the inclusive scan of the 16 elements, then carry16(carry); *total = what scan16 returned (the lane's sum before the carry)
int fd_scan16(int E, uint32_t* w, uint64_t carry, uint64_t* total) {
    switch (E) {
        case 1: *total = d::scan16<1>(w); d::carry16<1>(w, carry); return 0;
        case 2: *total = d::scan16<2>(w); d::carry16<2>(w, carry); return 0;
        case 4: *total = d::scan16<4>(w); d::carry16<4>(w, carry); return 0;
        case 8: *total = d::scan16<8>(w); d::carry16<8>(w, carry); return 0;
        default: return -1;
    }
}

uint32_t fd_restart_index(uint64_t e0) { return d::restart_index(e0); }
uint32_t fd_restart(void) { return d::RESTART; }
uint32_t fd_add8(uint32_t a, uint32_t b) { return d::add8(a, b); }
uint32_t fd_sub8(uint32_t a, uint32_t b) { return d::sub8(a, b); }
uint32_t fd_add16(uint32_t a, uint32_t b) { return d::add16(a, b); }
uint32_t fd_sub16(uint32_t a, uint32_t b) { return d::sub16(a, b); }

}  // extern "C"
