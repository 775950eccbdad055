// lz4_device.h -- kernel argument blocks and launch entry points shared by the HIP kernels
// and the host C ABI (capi.cpp; its context and host-only helpers: lz4_ctx.h).  Device-side status codes mirror include/lz4flex_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "paged_range.h" // the records of lz4flex_paged_read_ranges (plain integers, host and device)
#include "paged_append.h" // the record of lz4flex_paged_append (plain integers, host and device)
#include "lz4_route.h"  // PCD_PAIR_MAX_BLOCKS, the DISPATCH_* batch sizes and decode_route / encode_route: which kernel a batch takes (host-only, plain integers)

#define LZ4FLEX_DEV_E_OUTPUT_TOO_SMALL 1
#define LZ4FLEX_DEV_E_LITERAL_OUT_OF_BOUNDS 2
#define LZ4FLEX_DEV_E_EXPECTED_ANOTHER_BYTE 3
#define LZ4FLEX_DEV_E_OFFSET_ZERO 4
#define LZ4FLEX_DEV_E_OFFSET_OUT_OF_BOUNDS 5
#define LZ4FLEX_DEV_E_UNSUPPORTED 68        // lz4_packed.hip: a raw block that decompresses to more than the decoders' u32 out_cap holds
#define LZ4FLEX_DEV_E_INVALID_ARG 64        // a sink position behind the sink's end (out_pos > out_cap): the reference panics there

namespace lz4flex_range { struct RangeRec; }   // frame_range.h

namespace lz4flex_dev {

// All pointers are device pointers.
struct DecompressArgs {
    const uint8_t* in_base;
    const uint64_t* in_off;
    const uint32_t* in_len;
    uint8_t* out_base;
    const uint64_t* out_off;
    const uint32_t* out_cap;
    const uint32_t* out_pos;   // nullable: initial sink position (prefix mode of Linked frames)
    const uint8_t* dict_base;  // nullable: external dictionaries
    const uint64_t* dict_off;
    const uint32_t* dict_len;
    uint32_t* out_len;
    int32_t* status;
    uint64_t* detail;          // nullable: 2 per block (expected, actual)
    uint32_t n;
    int32_t only_status;       // lz4_decompress_blocks_kernel: 0 = every block, else only blocks whose status equals it (second pass)
    // lz4_decompress_pcd_kernel with out_pos: nullable; n words, zero before the launch.  Set => the batch is a CHAIN: the blocks share
    // one output region and block i's prefix [.., out_pos[i]) is what blocks 0..i-1 of this batch write (Linked frames,
    // src/frame/decompress.rs:195-222,280-306).  chain_done[i] becomes 1 (done, and every block before it) or 2 (given up).
    uint32_t* chain_done;
    // with chain_done: nullable; n words.  Set => the batch holds SEVERAL chains (N Linked frames side by side): block i's predecessor
    // is block chain_prev[i] (< i), 0xFFFFFFFF = the first block of its chain (nothing of the batch lies before it).  Null: i - 1.
    const uint32_t* chain_prev;
    uint32_t n_chains;         // with chain_prev: the number of chains (0 = unknown); picks the workgroup size (lz4_route.h decode_route)
    // lz4_decompress_pcd_kernel: nullable.  Set (n <= PCD_PAIR_MAX_BLOCKS, the first 64 n bytes zero before the launch) => every block
    // gets TWO workgroups: one parses its tiles and hands the token lists over through this workspace, the other copies
    // (lz4_decompress_pcd.hip "roles"); decompress_pcd_pair_ws_bytes() bytes
    uint8_t* pair_ws;
    // lz4_decompress_pcd_kernel, tests only: block debug_giveup - 1 of a chained batch gives up as if a wait had timed out (0: none)
    uint32_t debug_giveup;
};
size_t decompress_pcd_pair_ws_bytes();

struct CompressArgs {
    const uint8_t* in_base;
    const uint64_t* in_off;
    const uint32_t* in_len;
    const uint32_t* flags;     // nullable
    uint8_t* out_base;
    const uint64_t* out_off;
    const uint32_t* out_cap;
    uint32_t* out_len;
    int32_t* status;
    uint32_t n;
    uint32_t slide;            // throughput encoder: 0, or the bytes the windows of a block longer than 64 KiB advance by (32 768 or 49 152; lz4_compress_wave.hip Item)
    uint32_t sub;              // throughput encoder: 2 / 4 = blocks of at most 64 KiB are cut into that many sub-windows (small batches: lz4_compress_wave.hip Item::sub); else one window
    // nullable (all three or none): per-block external dictionaries (lz4flex_compress_batch_ex); dict_len[i] == 0 = block i has none.
    // Throughput encoder: the dictionary's last min(dict_len, 32 KiB) bytes are the block's history (lz4_compress_wave.hip Item);
    // reference-exact encoder: lz4_compress_blocks_kernel reads dict_len alone and leaves a block with dict_len[i] != 0 to the chain
    // kernel (launch_compress_exact; for a dictionary set dict_len is that launcher's one word per block).  Which dictionary a block
    // has when the batch has a shared one or a set: DictSource / block_dict below
    const uint8_t* dict_base;
    const uint64_t* dict_off;
    const uint32_t* dict_len;
    uint8_t* stage;            // throughput encoder: the workgroups' staging slots (set by launch_compress_wave)
};
// lz4flex_compress_batch_shared_dict: ONE dictionary of `len` bytes (device memory) for every block of the batch; the batch itself has
// no per-block dictionaries and no flags.  Throughput encoder: what the indexer does to the dictionary's tail is done once per call
// (lz4_compress_wave.hip, the digest); use 0 = every item takes the per-block path instead.  hs / keep / digest are set by launch_compress_wave.
struct SharedDictArgs {
    const uint8_t* dict;
    uint32_t len;
    uint32_t use;
    uint32_t hs;
    uint32_t keep;
    uint8_t* digest;
};

// A dictionary set (lz4flex_dict_set): K dictionaries in device memory the set owns, prepared once.  One record per dictionary:
struct DictSetRec {
    const uint8_t* end;        // behind the last of the `kept` bytes the set holds of it
    uint8_t* digest;           // its digest for the throughput encoder (compress_wave_digest_bytes() bytes; lz4_compress_wave.hip DG_*)
    uint32_t len;              // the caller's length, untruncated (reference-exact mode picks its table kind from it); 0 = no dictionary
    uint32_t kept;             // min(len, 65 536): an offset is at most 65 535
    uint32_t h, hs;            // throughput encoder: min(len, 32 768), and the positions the digest covers (0: no item starts from it)
};
// a batch's view of a set: block i has dictionary table[dict_id[i]]; DICT_ID_NONE = none; any other id >= k: the block is refused
// (status LZ4FLEX_E_INVALID_ARG, out_len 0, nothing written)
constexpr uint32_t DICT_ID_NONE = 0xFFFFFFFFu;
struct DictSetArgs {
    const DictSetRec* table;   // the front of the set's one allocation: every record's bytes lie behind it (launch_compress_exact's offsets count from here)
    const uint32_t* dict_id;
    uint32_t k;
    uint32_t use;              // throughput encoder: 0 = no item starts from a digest ("compress_shared_dict" 0)
    uint32_t* counter;         // throughput encoder: the items that started from a digest are counted here (the set's word)
};
// block b's dictionary: false = a refused id; dl == 0 = none
__device__ __forceinline__ bool dict_set_find(const DictSetArgs& st, uint32_t b, const uint8_t*& dict, uint32_t& dl) {
    const uint32_t id = st.dict_id[b];
    dict = nullptr; dl = 0u;
    if (id == DICT_ID_NONE) return true;
    if (id >= st.k) return false;
    const DictSetRec r = st.table[id];
    dict = r.end - r.kept; dl = r.kept;
    return true;
}
// The decode kernels' view of where a batch's dictionaries come from, a type per kind (a run-time ladder costs them instructions):
// NoDict, OneDict -- every block has the ONE dictionary dict[0, dict_len) (device memory, dict_len != 0) -- or DictSetArgs.  dict_find:
// block b's dictionary whatever the kind, as dict_set_find gives it
struct NoDict {};
struct OneDict { const uint8_t* dict; uint32_t dict_len; };
__device__ __forceinline__ bool dict_find(const NoDict&, uint32_t, const uint8_t*& dict, uint32_t& dl) { dict = nullptr; dl = 0u; return true; }
__device__ __forceinline__ bool dict_find(const OneDict& o, uint32_t, const uint8_t*& dict, uint32_t& dl) { dict = o.dict; dl = o.dict_len; return true; }
__device__ __forceinline__ bool dict_find(const DictSetArgs& st, uint32_t b, const uint8_t*& dict, uint32_t& dl) { return dict_set_find(st, b, dict, dl); }

// The dictionaries of a batch, in both directions: a set (has_set), else the batch's one dictionary (shared, shared_len bytes of device
// memory), else -- neither -- CompressArgs / DecompressArgs::dict_* where the batch has them.  The encoders' kernels read it
// (block_dict); for the decoders it is a host-side descriptor that picks the kernel instance (NoDict / OneDict / DictSetArgs above).
struct DictSource {
    const uint8_t* shared;
    uint32_t shared_len;
    uint32_t has_set;
    DictSetArgs set;
};
// Block b's dictionary: `end` is behind its last byte, `kept` of the bytes in front of `end` exist (a set keeps at most 64 KiB),
// `len` is the caller's length, untruncated; len == 0 = the block has none.  refused: an id the set does not have, or a per-block
// dictionary together with a non-zero flag word (frame flags or history bits) -- status LZ4FLEX_E_INVALID_ARG, out_len 0, nothing written.
struct BlockDict { bool refused; const uint8_t* end; uint32_t kept, len; };
__device__ __forceinline__ BlockDict block_dict(const CompressArgs& a, const DictSource& d, uint32_t b) {
    BlockDict r{false, nullptr, 0u, 0u};
    if (d.has_set) {
        const uint32_t id = d.set.dict_id[b];
        if (id == DICT_ID_NONE) return r;
        if (id >= d.set.k) { r.refused = true; return r; }
        const DictSetRec t = d.set.table[id];
        r.end = t.end; r.kept = t.kept; r.len = t.len;
    } else if (d.shared) {
        r.end = d.shared + d.shared_len; r.kept = r.len = d.shared_len;
    } else if (a.dict_len) {
        r.kept = r.len = a.dict_len[b];
        r.end = a.dict_base + a.dict_off[b] + r.len;
        r.refused = r.len != 0u && a.flags != nullptr && a.flags[b] != 0u;
    }
    return r;
}
// The one-block chain of compress_into_with_dict (compress.rs:554-583) as a chain record (Rec: lz4_compress.hip ChainBlock, the header's
// lz4flex_chain_block): the table kind from the UNtruncated dictionary length, the dictionary's last 64 KiB kept, input_stream_offset =
// their length.  dict_end: the offset behind the dictionary's last byte, in whatever dict_off indexes.
template <typename Rec>
__host__ __device__ inline Rec dict_chain_record(uint64_t in_off, uint32_t in_len, uint64_t dict_end, uint64_t dict_len) {
    const uint32_t kept = dict_len > 65536u ? 65536u : (uint32_t)dict_len;
    // {in_off, dict_off, in_len, in_pos, dict_len, so, repos, flags}
    return Rec{in_off, dict_end - kept, in_len, 0u, kept, kept, 0u, (dict_len + in_len < 65535u ? 1u : 0u) | 2u};
}

// plan / replay decoder (lz4_decompress_plan.hip, lz4_decompress_replay.hip; record format: lz4_plan_common.h)
namespace plan { struct BlockPlan; }
struct ReplayArgs {
    const uint8_t* in_base;
    uint8_t* out_base;
    const plan::BlockPlan* plans;   // n per-block headers
    const uint32_t* words;          // the plan array
    uint32_t n;
    uint32_t max_turns;             // no block's plan is longer than this many turns (a plan without its K_END must not hang the kernel)
};
hipError_t launch_replay(const ReplayArgs& a, hipStream_t s);
struct PlanArgs {
    const uint8_t* in_base;
    const uint64_t* in_off;
    const uint32_t* in_len;
    const uint64_t* out_off;
    const uint32_t* out_cap;
    plan::BlockPlan* plans;         // n per-block headers (written)
    uint32_t* words;                // the plan array: slot_words per block (written)
    uint32_t* out_len;
    int32_t* status;                // 0, or redo_code: the block has no plan (irregular) and is left to the reference-order kernel
    uint32_t n;
    uint32_t slot_words;
    int32_t redo_code;
};
size_t plan_slot_words();
hipError_t launch_plan(const PlanArgs& a, hipStream_t s);

// The decoders in the reference's check order (lz4_decompress.hip): a.only_status 0 = every block, else the marked ones.  The plain
// form -- DecompressArgs's own per-block dictionaries, prefixes, lanes_per_block lanes a block:
hipError_t launch_decompress(const DecompressArgs& a, int lanes_per_block, hipStream_t s);
// A batch's FORM is (d, partial).  d: no dictionary source, ONE dictionary for every block (lz4flex_decompress_batch_shared_dict) or block
// b's looked up in a set (_dict_set: a block without one decodes in the same launch, a refused id is LZ4FLEX_E_INVALID_ARG, out_len 0,
// nothing written); OffsetOutOfBounds is offset > produced + dict_len.  partial (lz4flex_decompress_batch_partial*): a.out_cap[b] is block
// b's TARGET -- the first min(size, target) bytes, no OutputTooSmall, no detail, nothing stored at or behind out_off[b] + target.
// The form (no source, not partial) is the plain one above; every other form has sixteen lanes a block whatever lanes_per_block says.
hipError_t launch_decompress(const DecompressArgs& a, const DictSource& d, bool partial, int lanes_per_block, hipStream_t s);
// one block per wavefront, one LANE PER SEQUENCE (lz4_decompress_seq.hip, round 6), every form: speculative part walks give the token
// positions, 64 sequences at a time are placed by a prefix sum and copied by their lanes; irregular blocks are left with status
// redo_code (a refused id gets its final status here).  The second pass of a form is launch_decompress with the same (d, partial) and
// only_status = redo_code.
hipError_t launch_decompress_seq(const DecompressArgs& a, const DictSource& d, bool partial, int32_t redo_code, hipStream_t s);
// What both refuse (hipErrorInvalidValue): a dictionary source or partial together with a.dict_base, a.out_pos or a.chain_done; a shared
// pointer with length 0; a set without table or dict_id.  (The plain sequence form refuses a.dict_base and a.chain_done: a prefix is fine there.)
inline bool decode_form_ok(const DecompressArgs& a, const DictSource& d, bool partial) {
    if (!d.has_set && d.shared == nullptr && !partial) return true;
    if (a.dict_base != nullptr || a.out_pos != nullptr || a.chain_done != nullptr) return false;
    if (d.has_set) return d.set.table != nullptr && d.set.dict_id != nullptr;
    return d.shared == nullptr || d.shared_len != 0u;
}
// the second pass of a CHAINED batch: the blocks whose status equals a.only_status, one after the other in chain order (one wavefront)
hipError_t launch_decompress_chain_redo(const DecompressArgs& a, hipStream_t s);
hipError_t launch_decompress_split(const DecompressArgs& a, hipStream_t s, int blocks_per_wg = 0);   // parser / copier wavefronts, no dict/prefix
// parser -> emitter -> quad wavefronts (lz4_decompress_fused.hip: the split decoder's parser, the replay decoder's copy engine, no dict/prefix);
// blocks of 512 KiB or more are left with status redo_code for a second pass of launch_decompress.  -DLZ4FLEX_TOOLS builds only (round 6)
hipError_t launch_decompress_fused(const DecompressArgs& a, int32_t redo_code, hipStream_t s);
// one WORKGROUP per block, token chain and copies parallel inside the block (lz4_decompress_pcd.hip: few, large blocks); irregular
// blocks are left with status redo_code like behind launch_decompress_seq.  test_geometry: tiny tiles / batches (tests only)
hipError_t launch_decompress_pcd(const DecompressArgs& a, int32_t redo_code, hipStream_t s, int geometry = 0);   // 0 production (1 024 lanes), 1 tests, 2 / 3 medium batches (256 / 512 lanes)
// the reference-exact block encoder (lz4_compress.hip): lanes per block (8 or 16), big: blocks may exceed 64 KiB (u32 table entries),
// emitter: a second wavefront writes the output (the product; without it: -DLZ4FLEX_ALL_VARIANTS builds, else hipErrorInvalidValue)
hipError_t launch_compress(const CompressArgs& a, int lanes, bool big, bool emitter, hipStream_t s);
// throughput ("wave") encoder, lz4_compress_wave.hip: persistent workgroups, `workspace` holds
// compress_wave_workspace_bytes(n_workgroups) bytes (cand[] slots + segment bodies, L2 / Infinity Cache resident)
size_t compress_wave_workspace_bytes(int n_workgroups);
// where the last shared-dictionary launch on `workspace` counts the items whose first window started from the digest (device memory)
const uint32_t* compress_wave_shared_counter(const void* workspace, int n_workgroups);
hipError_t launch_compress_wave(const CompressArgs& a, void* workspace, int n_workgroups, hipStream_t s,
                                unsigned long long* prof = nullptr,    // prof: 32 cycle counters (tools; lz4_compress_wave.hip wave_body), nullable
                                bool carry_wait = true,                // tests: false = a window that has to wait for its predecessor gives up at once
                                const SharedDictArgs* shared_dict = nullptr,    // nullable: the batch's one dictionary (the _shared_ kernels)
                                const DictSetArgs* dict_set = nullptr);         // nullable (not with shared_dict): a dictionary per block out of a set (the _set_ kernels)
// compress_mode 2 ("high", lz4_compress_high.hip): independent blocks without a dictionary, a.flags / slide / sub / dictionaries are not
// read; the bytes are tests/sim/high_encoder_model.c's for (block, depth).  Persistent workgroups, one per block at a time, each with a
// slice of `workspace` (compress_high_workspace_bytes(g) bytes for g of them): at most max_workgroups and as many as workspace_bytes holds
// parse ("compress_parse"): 0 = the lazy parse, 1 = the optimal one (tests/sim/high_optimal_model.c's bytes, all three forms; kernels of
// its own, the same workspace)
size_t compress_high_workspace_bytes(int n_workgroups);
hipError_t launch_compress_high(const CompressArgs& a, void* workspace, size_t workspace_bytes, int max_workgroups, uint32_t depth, uint32_t parse, hipStream_t s);
// its dictionary form ("compress_high_dict" 1): the bytes are tests/sim/high_dict_model.c's for (block, dictionary, depth).  Block b's
// dictionary is block_dict(a, d, b)'s (a refused block: status LZ4FLEX_E_INVALID_ARG, out_len 0, nothing written); a block without one,
// or with one of less than 4 bytes, gets the plain form's bytes.  use_digest (the shared dictionary only): a kernel in front sorts the
// dictionary tail's positions once, into the last slice of `workspace`, and every block sorts its own positions alone; else every block
// sorts the tail's with its own.
hipError_t launch_compress_high_dict(const CompressArgs& a, const DictSource& d, bool use_digest, void* workspace, size_t workspace_bytes,
                                     int max_workgroups, uint32_t depth, uint32_t parse, hipStream_t s);
// its history form ("compress_high_linked" 1): the dictionary form with block b's dictionary = the a.flags[b] >> 8 bytes of its own stream
// in front of it (LZ4FLEX_BLOCK_HISTORY), readable at a.in_base + a.in_off[b] - h; the flag word's low byte and a's dictionaries are not
// read, a.flags must not be null.  A block with h < 4 gets the plain form's bytes.
hipError_t launch_compress_high_linked(const CompressArgs& a, void* workspace, size_t workspace_bytes, int max_workgroups, uint32_t depth,
                                       uint32_t parse, hipStream_t s);
// a dictionary set's digests: bytes per dictionary, and the kernel that fills table[0 .. k)'s (a workgroup of one wavefront per
// dictionary; cand_scratch: compress_wave_digest_scratch_bytes() bytes per dictionary, dead behind the launch)
size_t compress_wave_digest_bytes();
uint32_t compress_wave_digest_hs(uint32_t h);     // the positions of an item with h bytes of dictionary in front that a digest covers
size_t compress_wave_digest_scratch_bytes();
hipError_t launch_dict_set_digests(const DictSetRec* table, uint32_t k, uint8_t* cand_scratch, hipStream_t s);

// chains of dependent blocks (dictionary / Linked frames); `blocks` is an array of the 40-byte ChainBlock
// records laid out as {u64 in_off, u64 dict_off, u32 in_len, in_pos, dict_len, so, repos, flags}.
// chain_first nullable: chain c starts at block c (one-block chains; chain_count[c] 0 = block c is not encoded, nothing written).
// dict_base nullable: dict_off indexes in_base
hipError_t launch_compress_chain(const uint8_t* in_base, const void* blocks, const uint32_t* chain_first,
                                 const uint32_t* chain_count, uint32_t n_chains, uint8_t* out_base,
                                 const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len, int32_t* status,
                                 uint32_t* tbl_state, hipStream_t s, const uint8_t* dict_base = nullptr);
// compress_mode 1 (reference-exact), independent blocks: launch_compress(a, lanes, big, emitter) for the blocks without a dictionary and -- !big:
// the caller promised blocks of at most 64 KiB -- INVALID_ARG for those among them that are longer; then, where the batch has
// dictionaries (a.dict_* or d), every block with one as a one-block chain of the chain kernel (dict_chain_record; refused: block_dict's
// refusals and in_len > 0x7FFFFFFF).  The records are built on the device in ws (ws_bytes bytes, read with dictionaries only), in pieces
// of as many blocks as it holds, at most max_piece of them (0: no limit; tests).
hipError_t launch_compress_exact(const CompressArgs& a, const DictSource& d, int lanes, bool big, bool emitter, void* ws,
                                 size_t ws_bytes, uint32_t max_piece, hipStream_t s);

hipError_t launch_xxh32_batch(const uint8_t* base, const uint64_t* off, const uint32_t* len, uint32_t n, uint32_t seed,
                              uint32_t* out, hipStream_t s);

// frame_kernels.hip: a rank's block range -> [header | payload | (checksum)]* on the device; seg_off holds n + 1 offsets
// (the last one = bytes written); pay_off / pay_len / sums are n-element scratch arrays, needed with block_checksums only
hipError_t launch_frame_assemble(const uint8_t* src_base, const uint64_t* src_off, const uint32_t* in_len, const uint8_t* comp_base,
                                 const uint64_t* comp_off, const uint32_t* comp_len, uint32_t n, int block_checksums, uint8_t* seg,
                                 uint64_t* seg_off, uint64_t* pay_off, uint32_t* pay_len, uint32_t* sums, hipStream_t s);
hipError_t launch_frame_walk(const uint8_t* f, uint64_t n, uint32_t hdr, uint32_t tail, uint32_t block_size, uint32_t max_blocks, uint64_t* off,
                             uint32_t* len, uint32_t* info, hipStream_t s);
// many frames at once (frame_many.cpp).  ManyStream: one stream to encode -- its blocks are [first, first + count) of the block arrays,
// its frame goes to out_base[out_off .. + out_cap); hdr = FrameInfo::write's bytes; flags bit 0 block checksums, bit 1 content checksum.
struct ManyStream { uint64_t out_off, out_cap; uint32_t first, count, hdr_len, flags; uint8_t hdr[24]; };
// ManyFrame: one frame to decode -- base[off .. + len), header of hdr_len bytes, table slots [slot, slot + slot_cap); skip: not walked
struct ManyFrame { uint64_t off, len; uint32_t hdr_len, block_size, flags, slot, slot_cap, skip; };
// verdict[s]: 0 written, 1 a block failed to compress, 2 the frame does not fit; frame_len[s] = bytes written.  dst_off (n_blocks) is
// scratch, pay_off / pay_len / sums (n_blocks) with block_checksums only, content_sum (n_streams) with content checksums only.
hipError_t launch_frame_many_assemble(const ManyStream* st, uint32_t n_streams, const uint8_t* src_base, const uint64_t* src_off, const uint32_t* in_len,
                                      const uint8_t* comp_base, const uint64_t* comp_off, const uint32_t* comp_len, const int32_t* comp_st, uint32_t n_blocks,
                                      int block_checksums, const uint32_t* content_sum, uint8_t* out_base, uint64_t* dst_off, uint64_t* pay_off,
                                      uint32_t* pay_len, uint32_t* sums, uint64_t* frame_len, int32_t* verdict, hipStream_t s);
hipError_t launch_frame_many_heads(const uint8_t* base, const uint64_t* off, const uint64_t* len, uint32_t n, uint8_t* heads, hipStream_t s);
hipError_t launch_frame_many_walk(const uint8_t* base, const ManyFrame* fr, uint32_t n, uint64_t* pay_off, uint32_t* word, uint32_t* info, hipStream_t s);
hipError_t launch_frame_sums_check(const uint8_t* base, const uint64_t* pay_off, const uint32_t* pay_len, const uint32_t* sums, uint32_t n, uint32_t* bad,
                                   hipStream_t s);
hipError_t launch_copy_batch(const uint8_t* src_base, const uint64_t* src_off, const uint32_t* len, uint8_t* dst_base, const uint64_t* dst_off,
                             uint32_t n, hipStream_t s);

// lz4_size_scan.hip (lz4flex_decompressed_size_batch): per block the bytes decompress_into would produce with an unbounded sink and
// history[i] (nullable: 0) bytes in front of the block, or its DecompressError; nothing but out_size / status is written.  A wavefront per
// block walks the token chain and sums the lengths; the blocks it leaves marked SIZE_SCAN_REDO are measured again in the reference's
// check order, a lane per block, behind it.  serial_only: that second pass for every block (tests).
constexpr int32_t SIZE_SCAN_REDO = 0x7F000003;
hipError_t launch_size_scan(const uint8_t* in_base, const uint64_t* in_off, const uint32_t* in_len, const uint32_t* history, uint32_t n,
                            uint64_t* out_size, int32_t* status, int serial_only, hipStream_t s);
// lz4_fit.hip (lz4flex_fit_batch, lz4flex_compress_batch_fit): every finished block blk_base + blk_off[i] (blk_len[i] bytes, decoding to the
// src_len[i] bytes at src_base + src_off[i]) cut to out_cap[i] bytes at out_base + out_off[i] by the fit rule (include/lz4flex_amd.h);
// in_used[i] = the source bytes the result decodes to.  A wavefront per block; the blocks it leaves marked FIT_REDO are taken again in the
// reference's check order, a lane per block, behind it.  gated: status[i] is read first and a block with status[i] != 0 keeps it (out_len
// and in_used 0: the encoder in front of this pass failed it).  serial_only 1: the second pass for every block (tests, A/B); 2: the first
// pass alone, a block it gives up keeps status FIT_REDO (the test hook "debug_fit_first_pass": which blocks does the wavefront pass finish?).
constexpr int32_t FIT_REDO = 0x7F000004;
struct FitArgs {
    const uint8_t* blk_base; const uint64_t* blk_off; const uint32_t* blk_len;
    const uint8_t* src_base; const uint64_t* src_off; const uint32_t* src_len;
    uint32_t n;
    uint8_t* out_base; const uint64_t* out_off; const uint32_t* out_cap;
    uint32_t* out_len; uint32_t* in_used; int32_t* status;
};
hipError_t launch_fit(const FitArgs& a, int gated, int serial_only, hipStream_t s);
// lz4_paged.hip (lz4flex_compress_paged): the step in front of, between and behind the rounds of a paged call, a lane per stream -- it
// commits the round behind it by the paged rule (include/lz4flex_amd.h) and lays out the next round's windows in the workspace; the
// round itself is the fit entry over w.w_off / w.w_len -> w.o_off / w.o_cap with its results in w.r_len / w.r_used / w.r_st.
enum : int { PAGED_NEXT = 0, PAGED_FIRST = 1, PAGED_LAST = 2 };     // bits.  FIRST: nothing to commit; LAST: nothing to lay out, what is live ends
struct PagedArgs {
    const uint64_t* in_off; const uint32_t* in_len; uint32_t n;
    uint32_t page_size, window_min, window_max;
    const uint64_t* page_off;                                       // n + 1, in entries
    uint32_t* page_len; uint32_t* page_src;                         // per entry
    uint32_t* n_pages; uint32_t* in_done; int32_t* status;          // per stream; n_pages and in_done are the loop's k and pos
};
// the arrays a paged call keeps in the caller's `work` (paged_work_bytes(n) bytes, any 8-byte aligned address)
struct PagedWork {
    void* packed;                                                   // the fit entry's own work area (packed_work_bytes(n))
    uint64_t* w_off; uint64_t* o_off;                               // n each: the round's windows and pages
    uint32_t* w_len; uint32_t* o_cap;
    uint32_t* r_len; uint32_t* r_used; int32_t* r_st;               // n each: the round's results
    uint32_t* win; uint32_t* live;                                  // n each: the window length W, 1 while the stream has rounds to come
};
size_t paged_work_bytes(uint32_t n);
PagedWork paged_work(void* work, uint32_t n);
hipError_t launch_paged_step(const PagedArgs& a, const PagedWork& w, int phase, hipStream_t s);
// lz4_paged_read.hip (lz4flex_paged_read_ranges): m byte ranges of paged streams, planned on the device.  Every pointer is device memory.
// The launches, in order: locate (a record per range; w.nb / w.hb: the sizes the two scans sum), launch_packed_scan twice (w.slot: align
// 1; w.head_off: align HEAD_ALIGN), plan (who is served and sound, then the items of the decode batches A -- max_items entries, sink: the
// output -- and B -- m entries, sink: the scratch -- and of the gather d_* from the scratch), the two partial decodes and the gather
// (capi.cpp), verdict (status / out_len per range).
struct PagedReadArgs {
    lz4flex_paged::Tables t;
    const uint32_t* range_stream; const uint32_t* range_off; const uint32_t* range_len; uint32_t m;
    const uint64_t* out_off; uint32_t* out_len; int32_t* status;
    uint32_t max_items; uint64_t scratch_cap;
};
// the arrays a call keeps in the caller's `work` (paged_read_work_bytes(m, max_items) bytes, any 8-byte aligned address)
struct PagedReadWork {
    lz4flex_paged::RangeRec* rec;                                   // m
    uint64_t* nb; uint64_t* hb;                                     // m each: touched pages, head bytes
    uint64_t* slot; uint64_t* head_off;                             // m + 1 each: their exclusive sums
    uint64_t* tiles;                                                // the scans' tile sums
    uint64_t* a_in; uint64_t* a_out; uint32_t* a_len; uint32_t* a_tgt; uint32_t* a_olen; int32_t* a_st;     // max_items each
    uint64_t* b_in; uint64_t* b_out; uint64_t* d_src; uint64_t* d_dst;                                     // m each
    uint32_t* b_len; uint32_t* b_tgt; uint32_t* b_olen; int32_t* b_st; uint32_t* d_len;                    // m each
};
size_t paged_read_work_bytes(uint32_t m, uint32_t max_items);
PagedReadWork paged_read_work(void* work, uint32_t m, uint32_t max_items);
hipError_t launch_paged_read_locate(const PagedReadArgs& a, const PagedReadWork& w, hipStream_t s);
hipError_t launch_paged_read_plan(const PagedReadArgs& a, const PagedReadWork& w, hipStream_t s);
hipError_t launch_paged_read_verdict(const PagedReadArgs& a, const PagedReadWork& w, hipStream_t s);
// lz4_paged_append.hip (lz4flex_paged_append): new bytes for any subset of n paged streams, planned on the device.  Every pointer is
// device memory.  The launches, in order: locate (a record per stream; w.need: the stage bytes the scan sums), launch_packed_scan (w.slot:
// align 1, the sizes are multiples of 64), emit (who is served; stage_off, tail_src; the tail items t_* of one partial decode, sink: the
// stage; the copy items c_* of the new bytes), the partial decode and the copy (capi.cpp), resume (the verdict of the tail decode, the
// rounds' state, round 1 in the PagedWork arrays and v_off / v_len, the in_off / in_len of the PagedArgs the rounds run with).
struct PagedAppendArgs {
    const uint64_t* add_off; const uint32_t* add_len; uint32_t n;
    uint32_t page_size, window_min, window_max;
    const uint64_t* page_off;                                       // n + 1, in entries
    uint32_t* page_len; uint32_t* page_src;                         // per entry
    uint32_t* n_pages; uint32_t* in_done; int32_t* status;          // per stream
    uint64_t stage_cap; uint64_t* stage_off; uint32_t* tail_src;    // per stream
};
// the arrays a call keeps in the caller's `work` (paged_append_work_bytes(n) bytes, any 8-byte aligned address)
struct PagedAppendWork {
    void* paged;                                                    // the rounds' own work area (paged_work(paged, n))
    lz4flex_paged::AppendRec* rec;                                  // n
    uint64_t* need;                                                 // n: stage bytes
    uint64_t* slot;                                                 // n + 1: their exclusive sums
    uint64_t* tiles;                                                // the scan's tile sums
    uint64_t* t_in; uint64_t* t_out; uint64_t* c_src; uint64_t* c_dst; uint64_t* v_off;                    // n each
    uint32_t* t_len; uint32_t* t_tgt; uint32_t* t_olen; int32_t* t_st; uint32_t* c_len; uint32_t* v_len;   // n each
};
size_t paged_append_work_bytes(uint32_t n);
PagedAppendWork paged_append_work(void* work, uint32_t n);
hipError_t launch_paged_append_locate(const PagedAppendArgs& a, const PagedAppendWork& w, hipStream_t s);
hipError_t launch_paged_append_emit(const PagedAppendArgs& a, const PagedAppendWork& w, hipStream_t s);
hipError_t launch_paged_append_resume(const PagedAppendArgs& a, const PagedAppendWork& w, bool no_rounds, hipStream_t s);
// lz4_packed.hip (lz4flex_decompress_batch_packed / lz4flex_compress_batch_packed): the output layout of a batch, computed on the device.
constexpr uint32_t PACKED_SCAN_TILE = 1024u;         // the sizes one workgroup scans ("packed_scan_tile")
// host helpers of the files that lay arrays out in a caller's `work` and launch a lane or a workgroup per item: an array's bytes rounded
// up to 256, the tile words launch_packed_scan needs for n sizes, the workgroups of a launch (the kernels stride over what is left)
inline size_t up256(size_t v) { return (v + 255u) & ~(size_t)255u; }
inline size_t scan_tiles(uint32_t n) { return (size_t)(((uint64_t)n + PACKED_SCAN_TILE - 1u) / PACKED_SCAN_TILE) + 2u; }
inline uint32_t grid_of(uint64_t groups) { return (uint32_t)(groups < (1u << 22) ? (groups ? groups : 1u) : (1u << 22)); }
enum : int {
    PACKED_SIZES_PREPENDED = 0,   // the LE u32 in front of every block; sh_off / sh_len receive the block behind it (in_len < 4: EXPECTED_ANOTHER_BYTE)
    PACKED_SIZES_GIVEN = 1,       // given[i]
    PACKED_SIZES_SCAN = 2,        // size / pre hold launch_size_scan's out_size / status (in place: failed blocks 0, more than 4 GiB - 1: UNSUPPORTED)
    PACKED_SIZES_SLOTS = 3,       // compress, scratch slots: get_maximum_output_size(in_len[i]) + extra
    PACKED_SIZES_PRODUCED = 4,    // compress, packed stream: given[i] (the encoder's out_len) + extra where given_st[i] == 0, else 0; pre is not written
};
// the arrays a packed call keeps in the caller's `work` (packed_work_bytes(n) bytes, any 8-byte aligned address)
struct PackedWork {
    uint64_t* size;       // n: slot sizes
    uint64_t* place;      // n: where the codec writes block i (0 for a block without room)
    uint64_t* aux_off;    // n + 1: PREPENDED: the blocks behind their prefixes; compress: the scratch slots' offsets
    uint64_t* tiles;      // the scan's tile sums
    uint32_t* aux_len;    // n: PREPENDED: the lengths behind the prefixes; compress: the scratch slots' capacities
    int32_t* pre;         // n: 0, or the status a block has before / instead of the codec's
};
size_t packed_work_bytes(uint32_t n);
PackedWork packed_work(void* work, uint32_t n);
hipError_t launch_packed_sizes(int mode, const uint8_t* in_base, const uint64_t* in_off, const uint32_t* in_len, const uint32_t* given,
                               const int32_t* given_st, uint32_t n, uint32_t extra, uint64_t* size, uint64_t* sh_off, uint32_t* sh_len,
                               int32_t* pre, hipStream_t s);
// off[0 .. n] = exclusive sums of the sizes, each rounded up to align (a power of two), off[n] the total.  Fit rule: block i fits iff
// off[i] + size[i] <= total_cap.  Nullable: place[i] = off[i] + shift (0 without room), cap[i] = size[i] - shift (0 without room),
// pre[i] = OUTPUT_TOO_SMALL without room (untouched otherwise).  tiles: n / PACKED_SCAN_TILE + 2 words of scratch
hipError_t launch_packed_scan(const uint64_t* size, uint32_t n, uint32_t align, uint64_t total_cap, uint32_t shift, uint64_t* tiles,
                              uint64_t* off, uint64_t* place, uint32_t* cap, int32_t* pre, hipStream_t s);
// decode: blocks with pre[i] != 0 get that status, out_len 0 and detail {off[i] + size[i], total_cap} (no room) or {0, 0}; the
// other blocks keep the decoder's detail if their status is OUTPUT_TOO_SMALL and get {0, 0} otherwise
hipError_t launch_packed_finish(const int32_t* pre, const uint64_t* size, const uint64_t* off, uint32_t n, uint64_t total_cap,
                                uint32_t* out_len, int32_t* status, uint64_t* detail, hipStream_t s);
// compress: block i with status 0 and room: [LE u32 in_len[i] (prefix = 4)] scratch[src_off[i] .. + size[i] - prefix) -> out + off[i],
// out_len[i] = size[i]; without room: status OUTPUT_TOO_SMALL; every block that is not copied: out_len 0
hipError_t launch_packed_gather(const uint8_t* scratch, const uint64_t* src_off, const uint64_t* size, const uint64_t* off,
                                const uint32_t* in_len, uint32_t n, uint32_t prefix, uint64_t total_cap, uint8_t* out, uint32_t* out_len,
                                int32_t* status, hipStream_t s);
// lz4_dict_train.hip (lz4flex_dict_train): a dictionary of at most dict_cap <= 65 536 bytes cut from the n samples, segments of k bytes
// (64 ... 2 048) chosen by the rule of tests/sim/dict_train_model.c.  Every pointer is device memory; work: dict_train_work_bytes(n) bytes,
// 8-byte aligned.  n == 0 or dict_cap == 0: *dict_len = 0, *status = 0 from a one-lane kernel.  Nothing is copied to the host.
size_t dict_train_work_bytes(uint32_t n);
hipError_t launch_dict_train(const uint8_t* in_base, const uint64_t* in_off, const uint32_t* in_len, uint32_t n, uint8_t* dict_out,
                             uint32_t dict_cap, uint32_t k, uint32_t* dict_len, int32_t* status, void* work, hipStream_t s);
// lz4_filter.hip (lz4flex_filter_batch, lz4flex_compress_batch_typed, lz4flex_decompress_batch_typed): the byte permutation `filter` for
// elements of `elem` bytes (1, 2, 4, 8), or its inverse, of every block: len[i] bytes from in_base + in_off[i] to out_base + out_off[i]
// (any alignment; the regions do not overlap).  gate: nullable; set => only the blocks with gate[i] == 0 (a decoder's status).  Nothing
// outside [off, off + len) is read or written.  One launch, no workspace.  `filter` may carry FILTER_DELTA: the difference stage in front
// of the permutation (inverse: the prefix sums behind its inverse), restarting every FILTER_TILE_ELEMS elements, in the same launch.
enum : int { FILTER_NONE = 0, FILTER_SHUFFLE = 1, FILTER_BITSHUFFLE = 2, FILTER_DELTA = 0x10 };     // the header's LZ4FLEX_FILTER_*; DELTA is a flag ORed into the other three
constexpr uint32_t FILTER_TILE_ELEMS = 1024u;        // the elements of one (block, tile) work item
struct FilterArgs {
    const uint8_t* in_base;
    const uint64_t* in_off;
    const uint32_t* len;
    const int32_t* gate;
    uint8_t* out_base;
    const uint64_t* out_off;
    uint32_t n;
    uint32_t bytewise;         // "filter_bytewise": 1 = every block by the narrow path (byte accesses)
};
hipError_t launch_filter(const FilterArgs& a, int filter, uint32_t elem, bool inverse, hipStream_t s);
// frame_range.hip (frame_index.cpp: lz4flex_frame_index_create / lz4flex_frame_read_ranges).
// The index: scan_len[b] = what launch_size_scan measures of walked block b (0 for a stored block), *first_bad = ~0; then size[b] (holding
// the scan's sizes) becomes the block's decoded bytes and *first_bad the first compressed block with scan_st != 0 or more than block_size bytes
hipError_t launch_frame_index_prep(const uint32_t* word, uint32_t n, uint32_t* scan_len, uint32_t* first_bad, hipStream_t s);
hipError_t launch_frame_index_sizes(const uint32_t* word, const int32_t* scan_st, uint32_t n, uint32_t block_size, uint64_t* size, uint32_t* first_bad,
                                    hipStream_t s);
// One pass of range reads: n_ranges records (frame_range.h RangeRec, slots ascending) over the index's device tables -> the items of two
// partial-decode batches (a_*: a slot per touched block, sink = the output; b_*: a slot per range, sink = scratch) and of two copy
// batches (c_*: per touched block, from the input; d_*: per range, from scratch).  Offsets are relative to the pass's bases.
struct FrameRangePlan {
    const lz4flex_range::RangeRec* rec;
    const uint64_t* content_off;
    const uint64_t* payload_off;
    const uint32_t* len_word;
    uint32_t n_ranges, n_slots;
    uint64_t *a_in, *a_out, *b_in, *b_out, *c_src, *c_dst, *d_src, *d_dst;
    uint32_t *a_len, *a_tgt, *b_len, *b_tgt, *c_len, *d_len;
};
hipError_t launch_frame_range_plan(const FrameRangePlan& p, hipStream_t s);
// the items' results -> per range status (0, -LZ4FLEX_FE_BLOCK_CHECKSUM, -LZ4FLEX_FE_DECOMPRESSION), out_len and the detail words;
// bad: nullable (launch_frame_sums_check's flags, a slot per touched block)
struct FrameRangeVerdict {
    const lz4flex_range::RangeRec* rec;
    const uint32_t* len_word;
    uint32_t n_ranges;
    const uint32_t* bad;
    const int32_t *a_st, *b_st;
    const uint32_t *a_tgt, *a_olen, *b_tgt, *b_olen;
    int32_t *status, *inner;
    uint64_t *out_len, *expected, *actual;
};
hipError_t launch_frame_range_verdict(const FrameRangeVerdict& v, hipStream_t s);
// DECODE_REDO: the status a first-pass decoder (sequence, workgroup, plan, fused) leaves on a block it does not decode: the host then runs a reference-order
// kernel with only_status = DECODE_REDO over the batch (capi.cpp launch_redo; which routes have one: lz4_route.h Redo)
constexpr int32_t DECODE_REDO = 0x7F000001;

// A launcher's opt-in to more than 64 KiB of dynamic LDS.  The attribute is per kernel and per device: allow() sets it for every
// kernel given on the current device the first time it runs there and remembers the device.  The first error is returned and the
// device stays unmarked.  One object per set of kernels -- a function-local static of the launcher (of each instantiation of a
// launcher template); two threads that race here both set the attribute, which is harmless.
struct LargeLds {
    unsigned long long have = 0ull;      // a bit per device
    template <class... K>
    hipError_t allow(size_t bytes, K... kernels) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        const unsigned long long bit = 1ull << (dev & 63);
        if (have & bit) return hipSuccess;
        for (const void* k : {reinterpret_cast<const void*>(kernels)...}) {
            const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
            if (e != hipSuccess) return e;
        }
        have |= bit;
        return hipSuccess;
    }
};

}  // namespace lz4flex_dev
