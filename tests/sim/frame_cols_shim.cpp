// frame_cols_shim.cpp -- C entry point over the frame layer's column sets (lz4_flex_amd/csrc/frame_cols.h) for tests/test_frame_cols_plan.py
// (ctypes): every set built from its counts over a 64-byte ColumnPlan, as frame_many.cpp, frame_index.cpp and sharded.cpp build them.
// Test infrastructure.  With -DFRAME_COLS_SHIM_MAIN: a stand-alone program over the same entry (sanitizer builds).
#define LZ4FLEX_STAGE_PLAN_ONLY
#include "../../lz4_flex_amd/csrc/frame_cols.h"

using namespace lz4flex_dev;

namespace {
template <size_t N> struct Elem { uint8_t b[N]; };      // stand-ins for the records lz4_device.h defines behind a HIP header
using Stream = Elem<56>;
using Frame = Elem<40>;

struct Out {
    uint64_t* at;
    uint32_t n = 0;
    void put() {}
    template <class T, class... Rest> void put(Col<T> c, Rest... rest) { at[n++] = c.at; put(rest...); }
};
}  // namespace

extern "C" {

// set: 0 many encode (nf, nb, chains) | 1 many heads (n) | 2 many walk (n, slots) | 3 many batch (ne, nr, nk, n) | 4 index scratch (mb, tiles)
//      5 index table (n) | 6 range pass (R, T) | 7 sharded encode (n) | 8 sharded decode (nc, nr, n)
// at[i]: where the set's i-th column starts, in declaration order (at most 32).  sum: up_bytes, total, and what the set's one "from this
// column to the end" fetch moves (range pass: from v_st; else 0).  Returns the number of columns, or -1 for a set it does not know.
int fc_plan(uint32_t set, const uint64_t* k, uint64_t* at, uint64_t* sum) {
    ColumnPlan p(64);
    Out o{at};
    sum[2] = 0;
    switch (set) {
        case 0: {
            const ManyEncodeCols<Stream> c(p, k[0], k[1], k[2] != 0);
            o.put(c.ms, c.soff, c.slen, c.in_off, c.comp_off, c.in_len, c.flags, c.comp_cap, c.cb, c.first, c.count, c.comp_len, c.comp_st, c.dst_off,
                  c.pay_off, c.pay_len, c.sums, c.csum, c.flen, c.verdict);
            break;
        }
        case 1: { const ManyHeadCols c(p, k[0]); o.put(c.off, c.len, c.heads); break; }
        case 2: { ManyWalkCols<Frame> c(p, k[0]); c.slots(p, k[1], k[0]); o.put(c.fr, c.pay, c.word, c.info); break; }
        case 3: {
            const ManyBatchCols c(p, k[0], k[1], k[2], k[3]);
            o.put(c.in, c.out, c.len, c.cap, c.pos, c.prev, c.rin, c.rout, c.rlen, c.poff, c.plen, c.olen, c.st, c.det, c.psum, c.bad, c.coff, c.clen, c.csum);
            break;
        }
        case 4: {
            const IndexScratchCols c(p, k[0], k[1]);
            o.put(c.pay, c.word, c.info, c.scan_len, c.size, c.scan_st, c.bad, c.content, c.tiles, c.one);
            break;
        }
        case 5: { const IndexTableCols c(p, k[0]); o.put(c.content, c.pay, c.word); break; }
        case 6: {
            const RangePassCols c(p, k[0], k[1]);
            o.put(c.rec, c.a_in, c.a_out, c.a_len, c.a_tgt, c.a_olen, c.a_st, c.c_src, c.c_dst, c.c_len, c.k_sum, c.k_bad, c.b_in, c.b_out, c.b_len, c.b_tgt,
                  c.b_olen, c.b_st, c.d_src, c.d_dst, c.d_len, c.v_st, c.v_inner, c.v_len, c.v_exp, c.v_act);
            sum[2] = p.from(c.v_st);
            break;
        }
        case 7: { const ShardEncodeCols c(p, k[0]); o.put(c.in_off, c.comp_off, c.seg_off, c.in_len, c.cap, c.clen, c.st, c.fl, c.scr); break; }
        case 8: {
            const ShardDecodeCols c(p, k[0], k[1], k[2]);
            o.put(c.cin, c.cout, c.rin, c.rout, c.poff, c.clen, c.ccap, c.rlen, c.plen, c.colen, c.cst, c.psum, c.bad);
            break;
        }
        default: return -1;
    }
    sum[0] = p.up_bytes; sum[1] = p.total();
    return (int)o.n;
}

// a typed view over memory laid out by a plan: byte offset of ColumnPlan::view(base, column) from base
uint64_t fc_view_offset(uint64_t col_at) {
    static uint8_t base[1];
    return (uint64_t)((uint8_t*)ColumnPlan::view(base, Col<uint64_t>{(size_t)col_at, 0}) - base);
}

}  // extern "C"

#ifdef FRAME_COLS_SHIM_MAIN
#include <cstdio>
// every set at one shape with all groups present and at one with every optional group empty: prints what the test's tables hold
int main() {
    const uint64_t shapes[2][9][4] = {
        {{3, 9, 1, 0}, {3, 0, 0, 0}, {3, 11, 0, 0}, {7, 2, 9, 3}, {1030, 3, 0, 0}, {9, 0, 0, 0}, {3, 5, 0, 0}, {5, 0, 0, 0}, {4, 1, 5, 0}},
        {{2, 0, 0, 0}, {1, 0, 0, 0}, {1, 0, 0, 0}, {0, 0, 0, 1}, {1, 2, 0, 0}, {0, 0, 0, 0}, {1, 0, 0, 0}, {1, 0, 0, 0}, {0, 0, 0, 0}}};
    for (const auto& shape : shapes)
        for (uint32_t set = 0; set < 9; set++) {
            uint64_t at[32], sum[3];
            const int n = fc_plan(set, shape[set], at, sum);
            if (n < 0) return 1;
            printf("set %u:", set);
            for (int i = 0; i < n; i++) printf(" %llu", (unsigned long long)at[i]);
            printf(" | up %llu total %llu tail %llu\n", (unsigned long long)sum[0], (unsigned long long)sum[1], (unsigned long long)sum[2]);
        }
    uint64_t at[32], sum[3];
    return fc_plan(9, shapes[0][0], at, sum) == -1 && fc_view_offset(192) == 192 ? 0 : 1;
}
#endif
