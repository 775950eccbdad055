// frame_cols.h -- the descriptor and result columns of the frame layer's calls, by name: one small struct of Col<T> per call site,
// built from the counts over a ColumnPlan (lz4_host_stage.h) in the order the device copy has always had.  Pure arithmetic, no HIP header:
// tests/test_frame_cols_plan.py pins every start against tables written by hand (tests/sim/frame_cols_shim.cpp, g++).  The two records
// lz4_device.h defines behind a HIP header, ManyStream and ManyFrame, are template parameters whose size is asserted here.
// up: the host fills it and it goes up; down: behind the plan's up_bytes.  Which bytes a call really sends is said at the call site.
#pragma once
#include "../../include/lz4flex_amd.h"
#include "frame_range.h"
#include "lz4_host_stage.h"

namespace lz4flex_dev {

static_assert(sizeof(lz4flex_chain_block) == 40, "a chain block record is 40 bytes on both sides");
static_assert(sizeof(lz4flex_range::RangeRec) == 64, "a range record is 64 bytes on both sides");

// ---- frame_many.cpp compress_many_device: nf streams of nb blocks in all.  cb / first / count: the reference-exact encoder's chains
// (Linked frames in exact mode), else of no elements
template <class Stream> struct ManyEncodeCols {
    static_assert(sizeof(Stream) == 56, "ManyStream is 56 bytes on both sides");
    Col<Stream> ms;
    Col<uint64_t> soff;
    Col<uint32_t> slen;
    Col<uint64_t> in_off, comp_off;
    Col<uint32_t> in_len, flags, comp_cap;
    Col<lz4flex_chain_block> cb;
    Col<uint32_t> first, count;
    Col<uint32_t> comp_len;           // results
    Col<int32_t> comp_st;
    Col<uint64_t> dst_off, pay_off;
    Col<uint32_t> pay_len, sums, csum;
    Col<uint64_t> flen;
    Col<int32_t> verdict;
    ManyEncodeCols(ColumnPlan& p, size_t nf, size_t nb, bool chains)
        : ms(p.up<Stream>(nf)), soff(p.up<uint64_t>(nf)), slen(p.up<uint32_t>(nf)), in_off(p.up<uint64_t>(nb)), comp_off(p.up<uint64_t>(nb)),
          in_len(p.up<uint32_t>(nb)), flags(p.up<uint32_t>(nb)), comp_cap(p.up<uint32_t>(nb)), cb(p.up<lz4flex_chain_block>(chains ? nb : 0)),
          first(p.up<uint32_t>(chains ? nf : 0)), count(p.up<uint32_t>(chains ? nf : 0)), comp_len(p.down<uint32_t>(nb)),
          comp_st(p.down<int32_t>(nb)), dst_off(p.down<uint64_t>(nb)), pay_off(p.down<uint64_t>(nb)), pay_len(p.down<uint32_t>(nb)),
          sums(p.down<uint32_t>(nb)), csum(p.down<uint32_t>(nf)), flen(p.down<uint64_t>(nf)), verdict(p.down<int32_t>(nf)) {}
};

// ---- frame_many.cpp decompress_many_device, n frames.  H: where the frames lie, their first 32 bytes
struct ManyHeadCols {
    Col<uint64_t> off, len;
    Col<uint8_t> heads;
    ManyHeadCols(ColumnPlan& p, size_t n) : off(p.up<uint64_t>(n)), len(p.up<uint64_t>(n)), heads(p.down<uint8_t>(32 * n)) {}
};
// W: the frames, and -- slots(), once the frames' table slots are counted -- the block tables (info: 8 words per frame)
template <class Frame> struct ManyWalkCols {
    static_assert(sizeof(Frame) == 40, "ManyFrame is 40 bytes on both sides");
    Col<Frame> fr;
    Col<uint64_t> pay{};
    Col<uint32_t> word{}, info{};
    ManyWalkCols(ColumnPlan& p, size_t n) : fr(p.up<Frame>(n)) {}
    void slots(ColumnPlan& p, size_t slots, size_t n) { pay = p.down<uint64_t>(slots); word = p.down<uint32_t>(slots); info = p.down<uint32_t>(8 * n); }
};
// B: ne compressed blocks, nr stored ones, nk block checksums; det: 2 words per block; coff / clen: filled and sent late, for the
// content checksums
struct ManyBatchCols {
    Col<uint64_t> in{}, out{};
    Col<uint32_t> len{}, cap{}, pos{}, prev{};
    Col<uint64_t> rin{}, rout{};
    Col<uint32_t> rlen{};
    Col<uint64_t> poff{};
    Col<uint32_t> plen{};
    Col<uint32_t> olen{};             // results
    Col<int32_t> st{};
    Col<uint64_t> det{};
    Col<uint32_t> psum{}, bad{};
    Col<uint64_t> coff{};
    Col<uint32_t> clen{}, csum{};
    ManyBatchCols() = default;
    ManyBatchCols(ColumnPlan& p, size_t ne, size_t nr, size_t nk, size_t n)
        : in(p.up<uint64_t>(ne)), out(p.up<uint64_t>(ne)), len(p.up<uint32_t>(ne)), cap(p.up<uint32_t>(ne)), pos(p.up<uint32_t>(ne)),
          prev(p.up<uint32_t>(ne)), rin(p.up<uint64_t>(nr)), rout(p.up<uint64_t>(nr)), rlen(p.up<uint32_t>(nr)), poff(p.up<uint64_t>(nk)),
          plen(p.up<uint32_t>(nk)), olen(p.down<uint32_t>(ne)), st(p.down<int32_t>(ne)), det(p.down<uint64_t>(2 * ne)), psum(p.down<uint32_t>(nk)),
          bad(p.down<uint32_t>(nk)), coff(p.down<uint64_t>(n)), clen(p.down<uint32_t>(n)), csum(p.down<uint32_t>(n)) {}
};

// ---- frame_index.cpp index_build: scratch for a table of up to mb blocks (no host image; `tiles`: mb / PACKED_SCAN_TILE + 2), and the
// index's own copy of the n blocks it found
struct IndexScratchCols {
    Col<uint64_t> pay{};
    Col<uint32_t> word{}, info{}, scan_len{};
    Col<uint64_t> size{};
    Col<int32_t> scan_st{};
    Col<uint32_t> bad{};
    Col<uint64_t> content{}, tiles{};
    Col<uint8_t> one{};
    IndexScratchCols() = default;
    IndexScratchCols(ColumnPlan& p, size_t mb, size_t n_tiles)
        : pay(p.down<uint64_t>(mb)), word(p.down<uint32_t>(mb)), info(p.down<uint32_t>(4)), scan_len(p.down<uint32_t>(mb)), size(p.down<uint64_t>(mb)),
          scan_st(p.down<int32_t>(mb)), bad(p.down<uint32_t>(2)), content(p.down<uint64_t>(mb + 1)), tiles(p.down<uint64_t>(n_tiles)),
          one(p.down<uint8_t>(64)) {}
};
struct IndexTableCols {
    Col<uint64_t> content, pay;
    Col<uint32_t> word;
    IndexTableCols(ColumnPlan& p, size_t n) : content(p.down<uint64_t>(n + 1)), pay(p.down<uint64_t>(n)), word(p.down<uint32_t>(n)) {}
};

// ---- frame_index.cpp run_pass: R ranges over T item slots.  The records go up; a / c / k: the items' decode, copy and checksum
// arrays; b / d: the heads' decode and copy arrays; v: the verdicts, which come back in one copy
struct RangePassCols {
    Col<lz4flex_range::RangeRec> rec;
    Col<uint64_t> a_in, a_out;
    Col<uint32_t> a_len, a_tgt, a_olen;
    Col<int32_t> a_st;
    Col<uint64_t> c_src, c_dst;
    Col<uint32_t> c_len, k_sum, k_bad;
    Col<uint64_t> b_in, b_out;
    Col<uint32_t> b_len, b_tgt, b_olen;
    Col<int32_t> b_st;
    Col<uint64_t> d_src, d_dst;
    Col<uint32_t> d_len;
    Col<int32_t> v_st, v_inner;
    Col<uint64_t> v_len, v_exp, v_act;
    RangePassCols(ColumnPlan& p, size_t R, size_t T)
        : rec(p.up<lz4flex_range::RangeRec>(R)), a_in(p.down<uint64_t>(T)), a_out(p.down<uint64_t>(T)), a_len(p.down<uint32_t>(T)),
          a_tgt(p.down<uint32_t>(T)), a_olen(p.down<uint32_t>(T)), a_st(p.down<int32_t>(T)), c_src(p.down<uint64_t>(T)), c_dst(p.down<uint64_t>(T)),
          c_len(p.down<uint32_t>(T)), k_sum(p.down<uint32_t>(T)), k_bad(p.down<uint32_t>(T)), b_in(p.down<uint64_t>(R)), b_out(p.down<uint64_t>(R)),
          b_len(p.down<uint32_t>(R)), b_tgt(p.down<uint32_t>(R)), b_olen(p.down<uint32_t>(R)), b_st(p.down<int32_t>(R)), d_src(p.down<uint64_t>(R)),
          d_dst(p.down<uint64_t>(R)), d_len(p.down<uint32_t>(R)), v_st(p.down<int32_t>(R)), v_inner(p.down<int32_t>(R)), v_len(p.down<uint64_t>(R)),
          v_exp(p.down<uint64_t>(R)), v_act(p.down<uint64_t>(R)) {}
};

// ---- sharded.cpp, a rank's n blocks.  Encode: everything in front of the assembler's scratch goes up (seg_off: n + 1 sums); scr lies
// behind up_bytes so that one plan gives the device size -- its host bytes are never sent or read
struct ShardEncodeCols {
    Col<uint64_t> in_off, comp_off, seg_off;
    Col<uint32_t> in_len, cap, clen;
    Col<int32_t> st;
    Col<uint32_t> fl;
    Col<uint8_t> scr;
    ShardEncodeCols(ColumnPlan& p, size_t n)
        : in_off(p.up<uint64_t>(n)), comp_off(p.up<uint64_t>(n)), seg_off(p.up<uint64_t>(n + 1)), in_len(p.up<uint32_t>(n)), cap(p.up<uint32_t>(n)),
          clen(p.up<uint32_t>(n)), st(p.up<int32_t>(n)), fl(p.up<uint32_t>(n)), scr(p.down<uint8_t>(16 * n)) {}
};
// Decode: nc compressed and nr stored blocks of the n, every payload for the block checksums
struct ShardDecodeCols {
    Col<uint64_t> cin, cout, rin, rout, poff;
    Col<uint32_t> clen, ccap, rlen, plen;
    Col<uint32_t> colen;              // results
    Col<int32_t> cst;
    Col<uint32_t> psum, bad;
    ShardDecodeCols(ColumnPlan& p, size_t nc, size_t nr, size_t n)
        : cin(p.up<uint64_t>(nc)), cout(p.up<uint64_t>(nc)), rin(p.up<uint64_t>(nr)), rout(p.up<uint64_t>(nr)), poff(p.up<uint64_t>(n)),
          clen(p.up<uint32_t>(nc)), ccap(p.up<uint32_t>(nc)), rlen(p.up<uint32_t>(nr)), plen(p.up<uint32_t>(n)), colen(p.down<uint32_t>(nc)),
          cst(p.down<int32_t>(nc)), psum(p.down<uint32_t>(n)), bad(p.down<uint32_t>(n)) {}
};

}  // namespace lz4flex_dev
