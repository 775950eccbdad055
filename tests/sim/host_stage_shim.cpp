// host_stage_shim.cpp -- C entry point over the plan layer of lz4_flex_amd/csrc/lz4_host_stage.h for tests/test_host_stage_plan.py (ctypes).
// Test infrastructure.  With -DHOST_STAGE_SHIM_MAIN: a stand-alone program over the same entry (sanitizer builds).
#define LZ4FLEX_STAGE_PLAN_ONLY
#include "../../lz4_flex_amd/csrc/lz4_host_stage.h"

using namespace lz4flex_dev;

namespace {
template <size_t N> struct Elem { uint8_t b[N]; };

// a column of `count` elements of `size` bytes, declared the way capi.cpp declares it: up<T> / down<T>
size_t column(StagePlan& p, bool up, uint64_t size, uint64_t count, size_t* from) {
#define HS_COL(N) { const Col<Elem<N>> c = up ? p.up<Elem<N>>(count) : p.down<Elem<N>>(count); *from = c.at; return c.at; }
    switch (size) {
        case 1: HS_COL(1)
        case 4: HS_COL(4)
        case 8: HS_COL(8)
        case 40: HS_COL(40)
        default: return (size_t)-1;
    }
#undef HS_COL
}
}  // namespace

extern "C" {

// ops: n_ops triples (kind, a, b): 0 = up(element size a, count b), 1 = down(a, b), 2 = region(bytes a, slack b), 3 = columns(slack a).
// at[i]: where op i's column / region starts; room[i]: a region's room (0 for a column).
// sum: up_bytes, total, arena_bytes, desc.at, from(the first down column) (0 without one).  Returns 0, or -1 for an op it does not know.
int hs_plan(uint64_t align, const uint64_t* ops, uint32_t n_ops, uint64_t* at, uint64_t* room, uint64_t* sum) {
    StagePlan p((size_t)align);
    size_t first_down = (size_t)-1;
    for (uint32_t i = 0; i < n_ops; i++) {
        const uint64_t kind = ops[3 * i], a = ops[3 * i + 1], b = ops[3 * i + 2];
        room[i] = 0;
        if (kind == 0 || kind == 1) {
            size_t from = 0;
            const size_t v = column(p, kind == 0, a, b, &from);
            if (v == (size_t)-1) return -1;
            at[i] = v;
            if (kind == 1 && first_down == (size_t)-1) first_down = from;
        } else if (kind == 2 || kind == 3) {
            const Region r = kind == 2 ? p.region((size_t)a, (size_t)b) : p.columns((size_t)a);
            at[i] = r.at;
            room[i] = r.room;
        } else {
            return -1;
        }
    }
    sum[0] = p.up_bytes; sum[1] = p.total(); sum[2] = p.arena_bytes; sum[3] = p.desc.at;
    sum[4] = first_down == (size_t)-1 ? 0 : p.from(Col<uint8_t>{first_down, 0});
    return 0;
}

}  // extern "C"

#ifdef HOST_STAGE_SHIM_MAIN
#include <cstdio>
// the general batch path's declarations for 9 blocks with every optional column, and again with none: prints what the test's table holds
int main() {
    for (uint64_t opt = 0; opt < 2; opt++) {
        const uint64_t n = 9, o = opt ? 0 : n;
        const uint64_t ops[] = {0, 8, n, 0, 8, n, 0, 8, o, 0, 4, n, 0, 4, n, 0, 4, o, 0, 4, o, 0, 4, o, 0, 4, o, 1, 4, n, 1, 4, n, 1, 8, 2 * n,
                                2, 5000, 64, 2, 9001, 64, 2, opt ? 0u : 300u, 64, 3, 0, 0};
        const uint32_t n_ops = sizeof ops / sizeof ops[0] / 3;
        uint64_t at[16], room[16], sum[5];
        if (hs_plan(16, ops, n_ops, at, room, sum)) return 1;
        for (uint32_t i = 0; i < n_ops; i++) printf("%llu ", (unsigned long long)at[i]);
        printf("| up %llu total %llu arena %llu desc %llu from %llu\n", (unsigned long long)sum[0], (unsigned long long)sum[1],
               (unsigned long long)sum[2], (unsigned long long)sum[3], (unsigned long long)sum[4]);
    }
    return 0;
}
#endif
