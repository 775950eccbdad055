// lz4_route.h -- which decoder and which encoder a batch takes: pure functions of the context's settings and the batch's shape, on plain
// integers.  Host only, no HIP include: g++ compiles it alone (tests/sim/host_routes_shim.cpp; tests/test_host_routes.py holds the tables
// these functions have to give, written by hand).  capi.cpp computes a route once per batch and its launch code switches on it; the
// "decompress_variant" validity check and the "decoder_config_<i>" / "dispatch_threshold_<i>" lists of lz4flex_get_tuning are read off
// the tables here.  lz4_device.h includes this header: the kernels' launchers see the same constants.
#pragma once
#include <stdint.h>

namespace lz4flex_dev {

// The batch sizes at which decode_route changes decoder or geometry ("dispatch_threshold_<i>": DISPATCH_THRESHOLDS in this order).  The
// tests' decoder matrix is every threshold and its successor -- a threshold edit cannot leave a size class untested (a wrong result
// lived a round in batches of 5 121 ... 16 383 blocks because one geometry was never run on real data).
constexpr uint32_t PCD_PAIR_MAX_BLOCKS = 128u;       // <= : a workgroup-decoder batch may get two workgroups per block (DecompressArgs::pair_ws)
constexpr uint32_t DISPATCH_PCD_1024 = 256u;         // <= : a workgroup of 1 024 lanes per block (one per CU); also for large blocks and chains at any count
constexpr uint32_t DISPATCH_PCD_512 = 512u;          // <= : 512 lanes per block (two per CU)
constexpr uint32_t DISPATCH_PCD_256 = 640u;          // <= : 256 lanes per block (four per CU); up to here the default dispatch takes the workgroup decoder
// round 6: above, a wavefront per block and a lane per sequence (lz4_decompress_seq.hip) -- its time grows with the batch (16 wavefronts per
// CU: 4 096 blocks are one round), the split decoder's is one block's chain whatever the batch: JSON tiles 768 / 4 096 / 8 192 / 12 288 /
// 14 336 / 16 384 blocks 0.32 / 0.53 / 1.00 / 1.44 / 1.63 / 1.82 ms against 0.35 (256 lanes per block) / 1.01 / 1.63 / 1.64 / 1.65 / 1.67;
// text and log tiles are ahead at every size (16 384 blocks: 2.76 against 3.53, 1.57 against 2.25 ms) -- the threshold is the JSON one
// (profiles/r06_decoder_shapes.txt)
constexpr uint32_t DISPATCH_SEQ_MAX = 14336u;        // <= : a wavefront per block, a lane per sequence; above: the split decoder
constexpr uint32_t DISPATCH_SPLIT_FULL = 64u * 256u;  // (not a change of kernel: from here on every CU holds a workgroup of the split decoder; the tests want this size too)
constexpr uint32_t DISPATCH_THRESHOLDS[] = {PCD_PAIR_MAX_BLOCKS, DISPATCH_PCD_1024, DISPATCH_PCD_512, DISPATCH_PCD_256, DISPATCH_SEQ_MAX, DISPATCH_SPLIT_FULL};
// blocks per chained decode batch (LZ4FLEX_MEM_CHAINED): the context has one "done" word for each, frame_many.cpp cuts its batches to fit
constexpr uint32_t CHAIN_MAX_BLOCKS = 65536u;

// ---- decoders.  The values are the public "decompress_variant" numbers (include/lz4flex_amd.h).
enum Decoder : int {
    DEC_AUTO = 0,             // by batch shape
    DEC_REFERENCE = 1,        // the reference's order of checks, window in HBM / L2 (lz4_decompress.hip)
    DEC_SPLIT = 4,            // a lane per block parses, four copy (lz4_decompress_split.hip)
    DEC_WORKGROUP = 7,        // a workgroup per block (lz4_decompress_pcd.hip), 1 024 lanes
    DEC_WORKGROUP_TEST = 8,   //   ... its small test geometry
    DEC_PLAN = 9,             // plan / replay (lz4_decompress_plan.hip, lz4_decompress_replay.hip)
    DEC_WORKGROUP_256 = 10,   // a workgroup per block, 256 lanes
    DEC_WORKGROUP_512 = 11,   //   ... 512 lanes
    DEC_FUSED = 12,           // parser / emitter / quads (lz4_decompress_fused.hip)
    DEC_SEQUENCE = 13,        // a wavefront per block, a lane per sequence (lz4_decompress_seq.hip)
};
// The second pass behind a first-pass decoder (capi.cpp launch_redo): none, the marked blocks side by side, or -- a chain's marked
// blocks depend on each other -- one after the other in chain order
enum class Redo { None, Batch, ChainOrder };

// ONE table of what "decompress_variant" can be pinned to, in the order of "decoder_config_<i>" (variant * 1000 + parameter: the values
// "decompress_lanes" takes for variant 1, "decompress_blocks_per_wg" for variant 4, else 0).  tools_only: -DLZ4FLEX_TOOLS builds alone
// hold the kernel.  What the launch code needs of a variant stands beside it: the kernel family it runs (`runs`), the workgroup
// decoder's geometry (launch_decompress_pcd: 0 production, 1 tests, 2 / 3 = 256 / 512 lanes) and whether a second pass follows.
struct DecoderVariant {
    Decoder variant;
    int n_configs, config[3];
    bool tools_only;
    Decoder runs;
    int pcd_geometry;
    Redo redo;
};
constexpr DecoderVariant DECODER_VARIANTS[] = {
    {DEC_AUTO, 0, {}, false, DEC_AUTO, 0, Redo::None},
    {DEC_REFERENCE, 1, {16}, false, DEC_REFERENCE, 0, Redo::None},
    {DEC_SPLIT, 3, {8, 32, 64}, false, DEC_SPLIT, 0, Redo::None},
    {DEC_WORKGROUP, 1, {0}, false, DEC_WORKGROUP, 0, Redo::Batch},
    {DEC_WORKGROUP_TEST, 1, {0}, false, DEC_WORKGROUP, 1, Redo::Batch},
    {DEC_WORKGROUP_256, 1, {0}, false, DEC_WORKGROUP, 2, Redo::Batch},
    {DEC_WORKGROUP_512, 1, {0}, false, DEC_WORKGROUP, 3, Redo::Batch},
    {DEC_SEQUENCE, 1, {0}, false, DEC_SEQUENCE, 0, Redo::Batch},
    {DEC_PLAN, 1, {0}, true, DEC_PLAN, 0, Redo::Batch},
    {DEC_FUSED, 1, {0}, true, DEC_FUSED, 0, Redo::Batch},
};
// the table's row for v in this kind of build; null: "decompress_variant" refuses v (5 / 6, the wave decoder and its two-wavefront form,
// were replaced by 13 in round 6; 9 and 12 exist in tools builds only)
inline const DecoderVariant* decoder_variant(int v, bool tools) {
    for (const DecoderVariant& d : DECODER_VARIANTS)
        if (d.variant == v && (tools || !d.tools_only)) return &d;
    return nullptr;
}
// entry i of "decoder_config_<i>", -1 behind the last
inline int decoder_config(int i, bool tools) {
    for (const DecoderVariant& d : DECODER_VARIANTS) {
        if (d.tools_only && !tools) continue;
        if (i >= 0 && i < d.n_configs) return d.variant * 1000 + d.config[i];
        i -= d.n_configs;
    }
    return -1;
}

struct DecodeSettings {
    int dec_variant, dec_pcd_pair, dec_shared, dec_partial;    // "decompress_variant", "decompress_pcd_pair", "decompress_shared_dict", "decompress_partial"
    bool pair_ws;             // the context has the pair hand-over workspace
    bool tools;               // a -DLZ4FLEX_TOOLS build
    bool plan_fits;           // the batch's plans are addressable (BlockPlan's word indices are 32-bit)
};
struct DecodeShape {
    uint32_t n;
    bool big_blocks;          // LZ4FLEX_MEM_BIG_BLOCKS, or what a host batch's lengths say
    bool prefix;              // out_pos: the sinks hold bytes in front of the blocks
    bool chained;             // LZ4FLEX_MEM_CHAINED
    bool chain_prev;          // ... several chains side by side,
    uint32_t n_chains;        //     this many (0 = unknown)
    bool block_dicts;         // per-block dictionaries (lz4flex_decompress_batch_ex)
    bool dict_source, partial;   // the batch's form: a shared dictionary or a set; targets
};
// decoder: the family that runs -- DEC_REFERENCE (every block in the reference's order, no first pass), DEC_SPLIT, DEC_WORKGROUP,
// DEC_PLAN, DEC_FUSED or DEC_SEQUENCE
struct DecodeRoute {
    Decoder decoder;
    int pcd_geometry;
    bool pair;
    Redo redo;
};

// The decoder of one batch.
//  * A form with a dictionary source or targets: the sequence decoder -- a wavefront per block and a lane per sequence at every n (never
//    worse than sixteen serial lanes per block; a partial form's work is bounded by the target, not by the block) -- and a second pass,
//    unless "decompress_variant" is 1, or the form has a dictionary source and "decompress_shared_dict" is 0, or it is partial and
//    "decompress_partial" is 0: then the reference's order for every block.
//  * The plain form.  Per-block dictionaries, or variant 1 (a chain has no such form): the reference's order.  Else by batch shape
//    (tools/dec_shapes.py measures every decoder on every shape, profiles/r06_decoder_shapes.txt):
//      up to DISPATCH_PCD_256 blocks, or blocks known to be large: a whole WORKGROUP per block, token chain and copies parallel INSIDE the
//        block -- the decoder whose time for a block is not the length of the block's chain: 256 / 512 JSON blocks 0.14 / 0.23 ms,
//        256 x 4 MiB log blocks 4.7 ms, one 16 MiB block 14.6 ms;
//      up to DISPATCH_SEQ_MAX blocks: a WAVEFRONT per block, a lane per sequence (round 6: it replaced the wave decoder and its
//        two-wavefront form, 0.74 / 1.01 ms for 1 024 / 4 096 JSON blocks): 768 / 2 304 / 4 096 / 8 192 / 12 288 JSON blocks 0.32 / 0.41 /
//        0.53 / 1.00 / 1.44 ms, 4 096 text / log / incompressible blocks 0.88 / 0.49 / 0.30 ms;
//      larger batches: a LANE per block parses, four lanes copy: 1.63 - 1.67 ms for any batch of 5 121 ... 16 384 JSON blocks -- the
//        chain of one block.
inline DecodeRoute decode_route(const DecodeSettings& st, const DecodeShape& sh) {
    const DecodeRoute reference{DEC_REFERENCE, 0, false, Redo::None};
    if (sh.dict_source || sh.partial) {
        const bool first_pass = st.dec_variant != DEC_REFERENCE && (st.dec_shared || !sh.dict_source) && (st.dec_partial || !sh.partial);
        return first_pass ? DecodeRoute{DEC_SEQUENCE, 0, false, Redo::Batch} : reference;
    }
    if (sh.block_dicts || (st.dec_variant == DEC_REFERENCE && !sh.chained)) return reference;
    const bool chain = sh.chained && sh.n != 0;        // (an empty batch has no chain bracket)
    const bool automatic = st.dec_variant == DEC_AUTO;
    int v = !automatic ? st.dec_variant
                       : (sh.n <= DISPATCH_PCD_256 || sh.big_blocks) ? DEC_WORKGROUP : sh.n <= DISPATCH_SEQ_MAX ? DEC_SEQUENCE : DEC_SPLIT;
    const DecoderVariant* row = decoder_variant(v, st.tools);
    // (an explicit geometry holds for prefix / chained batches too)
    int geometry = row ? row->pcd_geometry : 0;
    // prefix mode (Linked frames): the workgroup decoder, or -- a batch whose prefixes are in memory already, not a CHAINED one -- the
    // sequence decoder (round 6)
    if (sh.prefix && v != DEC_WORKGROUP_TEST && !(v == DEC_SEQUENCE && !chain)) v = DEC_WORKGROUP;
    if (automatic && v == DEC_WORKGROUP) {
        // the workgroup decoder's geometry by batch size (lz4_decompress_pcd.hip GeoMid*: smaller workgroups, more of them per CU); large
        // blocks and chains keep the full workgroup (a chain is one block at a time, a large block wants the long tiles)
        if (!sh.big_blocks && !sh.prefix && sh.n > DISPATCH_PCD_1024) geometry = sh.n <= DISPATCH_PCD_512 ? 3 : 2;
        // several chains side by side (chain_prev): one block per chain is runnable at a time, so the CHAINS are what fills the chip --
        // tools/many_probe.py, 1 GiB of Linked JSON frames of 64 KiB blocks, 1 024 / 256 lanes per block: 256 chains 8.3 / 16.8 ms,
        // 1 024 chains 8.3 / 6.1, 4 096 chains 9.0 / 6.7, 64 chains 20.5 / 63
        if (chain && sh.chain_prev && sh.n_chains > DISPATCH_PCD_1024) geometry = sh.n_chains <= DISPATCH_PCD_512 ? 3 : 2;
    }
    if (v == DEC_PLAN && !st.plan_fits) v = DEC_SPLIT;     // (ADVICE r4): such a batch takes the split decoder
    // few LARGE blocks: a parser and a copier workgroup each (half the CUs would idle otherwise; a block of one tile has nothing to
    // overlap and would only pay the hand-over: 64 KiB JSON blocks 0.144 -> 0.156 ms).  "decompress_pcd_pair" 2 = always (tests)
    const bool pair = (v == DEC_WORKGROUP || v == DEC_WORKGROUP_TEST) && (st.dec_pcd_pair == 2 || (st.dec_pcd_pair == 1 && sh.big_blocks)) &&
                      st.pair_ws && sh.n <= PCD_PAIR_MAX_BLOCKS;
    row = decoder_variant(v, st.tools);
    // (a number this build has no first-pass kernel for -- the environment can still pin one -- is the split decoder's, as 4 is)
    if (!row || row->runs == DEC_AUTO || row->runs == DEC_REFERENCE) return {DEC_SPLIT, 0, false, Redo::None};
    return {row->runs, geometry, pair, chain && row->runs == DEC_WORKGROUP ? Redo::ChainOrder : row->redo};
}

// ---- encoders.  mode: the effective "compress_mode" (0 throughput, 1 reference-exact, 2 high); form: the high encoder's.
enum class HighForm { Plain, Dict, History };
struct EncodeSettings { int comp_mode, comp_high_dict, comp_high_linked; };     // "compress_mode", "compress_high_dict", "compress_high_linked"
struct EncodeShape {
    bool dicts;               // per-block dictionaries, a shared one or a set
    bool flags;               // the call has flag words (LZ4FLEX_BLOCK_HISTORY bits among them)
    bool linked_frame;        // the blocks are a Linked frame's (the frame layer's calls; a direct caller cannot say so)
};
struct EncodeRoute { int mode; HighForm form; };
// "compress_mode" 2 (high) encodes independent blocks: a call with dictionaries takes the dictionary form with "compress_high_dict" 1
// and the throughput encoder otherwise; one without dictionaries and with flags takes the history form with "compress_high_linked" 1
// (the LZ4FLEX_BLOCK_HISTORY bytes in front of a block are its dictionary) and the plain form otherwise -- but a Linked frame's blocks
// under "compress_high_linked" 0 are the throughput encoder's: their history bits are read there, the plain form would drop them.
inline EncodeRoute encode_route(const EncodeSettings& st, const EncodeShape& sh) {
    if (st.comp_mode != 2) return {st.comp_mode, HighForm::Plain};
    if (sh.linked_frame && !st.comp_high_linked) return {0, HighForm::Plain};
    if (sh.dicts) return st.comp_high_dict ? EncodeRoute{2, HighForm::Dict} : EncodeRoute{0, HighForm::Plain};
    return {2, sh.flags && st.comp_high_linked ? HighForm::History : HighForm::Plain};
}

}  // namespace lz4flex_dev
