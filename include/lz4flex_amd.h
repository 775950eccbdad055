/*
 * lz4flex_amd.h -- C ABI of the MI355X-native LZ4 block codec (drop-in boundary).
 *
 * lz4_flex has no FFI of its own: its boundary IS its public Rust API.  Each entry point
 * below names the lz4_flex item it replaces (paths relative to the lz4_flex v0.12.0 tree);
 * INTEGRATION.md shows the Rust `extern "C"` shim a maintainer would add on the reference
 * side.  Plain pointers and sizes only; no torch / C++ types.
 *
 * Every compute entry point runs hand-written HIP kernels on the GPU.  There is NO CPU
 * fallback: without a usable HIP device the calls return -LZ4FLEX_E_NO_DEVICE / -LZ4FLEX_E_HIP.
 *
 * Return convention for scalar calls: >= 0 is the byte count (Ok(usize)), < 0 is -code (Err).
 */
#ifndef LZ4FLEX_AMD_H
#define LZ4FLEX_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes ------------------------------------------------------------------------- */
/* block::DecompressError, variant order of src/block/mod.rs:82-98 */
#define LZ4FLEX_OK 0
#define LZ4FLEX_E_OUTPUT_TOO_SMALL 1       /* also block::CompressError::OutputTooSmall, mod.rs:103-106 */
#define LZ4FLEX_E_LITERAL_OUT_OF_BOUNDS 2
#define LZ4FLEX_E_EXPECTED_ANOTHER_BYTE 3
#define LZ4FLEX_E_OFFSET_ZERO 4
#define LZ4FLEX_E_OFFSET_OUT_OF_BOUNDS 5
/* frame::Error, src/frame/mod.rs:35-72 */
#define LZ4FLEX_FE_COMPRESSION 16
#define LZ4FLEX_FE_DECOMPRESSION 17
#define LZ4FLEX_FE_IO 18
#define LZ4FLEX_FE_UNSUPPORTED_BLOCKSIZE 19
#define LZ4FLEX_FE_UNSUPPORTED_VERSION 20
#define LZ4FLEX_FE_WRONG_MAGIC 21
#define LZ4FLEX_FE_RESERVED_BITS 22
#define LZ4FLEX_FE_INVALID_BLOCK_INFO 23
#define LZ4FLEX_FE_BLOCK_TOO_BIG 24
#define LZ4FLEX_FE_HEADER_CHECKSUM 25
#define LZ4FLEX_FE_BLOCK_CHECKSUM 26
#define LZ4FLEX_FE_CONTENT_CHECKSUM 27
#define LZ4FLEX_FE_SKIPPABLE_FRAME 28
#define LZ4FLEX_FE_DICTIONARY_NOT_SUPPORTED 29
#define LZ4FLEX_FE_CONTENT_LENGTH 30
#define LZ4FLEX_FE_OUTPUT_FULL 31          /* one-shot helpers only: caller's flat buffer too small */
/* library/runtime errors (API misuse or device failure; the reference would panic) */
#define LZ4FLEX_E_INVALID_ARG 64
#define LZ4FLEX_E_NO_DEVICE 65
#define LZ4FLEX_E_HIP 66
#define LZ4FLEX_E_NOMEM 67
#define LZ4FLEX_E_UNSUPPORTED 68         /* entry point declared but its GPU path is not built yet */

typedef struct lz4flex_err_detail {
    uint64_t expected; /* OutputTooSmall{expected}, ContentLengthError{expected}, SkippableFrame(len), ... */
    uint64_t actual;   /* OutputTooSmall{actual},   ContentLengthError{actual} */
    int32_t inner;     /* frame: block error code wrapped by DecompressionError */
    int32_t hip_error; /* hipError_t when the code is LZ4FLEX_E_HIP */
} lz4flex_err_detail;

/* ---- context ------------------------------------------------------------------------------ */
/* Owns the device workspace (the throughput encoder's 164 MiB of candidate slots and segment bodies and 32 MiB of staging slots
 * for dictionary items, allocated HERE so
 * that no compress call allocates; the staging arena and descriptor arrays of MEM_HOST calls) and a HIP stream.
 * One context per thread; distinct contexts are independent (reference: no global state, all fns reentrant).  MEM_DEVICE
 * compress batches of ONE context share its encoder workspace: the library orders them on the device (a batch enqueued on
 * another stream than the previous one waits for it), so they never overlap -- use one context per stream for concurrency.
 * The scalar calls below use a lazily created per-thread default context on the current HIP device. */
typedef struct lz4flex_ctx lz4flex_ctx;
int lz4flex_ctx_create(lz4flex_ctx **ctx, int device /* -1 = current */);
void lz4flex_ctx_destroy(lz4flex_ctx *ctx);
int lz4flex_device_count(void);
const char *lz4flex_version(void);
/* hash of the sources (csrc/ + include/ + compiler flags) this binary was built from; lz4_flex_amd/build.py
 * recomputes it from the tree, so a stale library is detectable */
const char *lz4flex_build_id(void);
/* The round of this header: 8.  Changes a caller built against an earlier header has to know: round 5 appended chain_prev / n_chains to
 * lz4flex_decompress_ext (read only for LZ4FLEX_MEM_DEVICE | LZ4FLEX_MEM_CHAINED batches; a struct of the four older members is fine for
 * every other call); round 6 removed "decompress_variant" 5 / 6 (the wave decoder; 13 took its place) and moved 12 to tools builds;
 * round 7 added lz4flex_decompressed_size_batch and the setting "size_scan_serial"; round 8 added lz4flex_compress_batch_ex
 * (per-block dictionaries for compressing, both compress modes) -- the context's device workspace grew by 64 KiB per encoder workgroup.
 * Later additions that change nothing for an existing call keep the number: lz4flex_compress_batch_shared_dict and the setting
 * "compress_shared_dict" came after round 8 (the workspace grew by 41 KiB per context), then lz4flex_decompress_batch_shared_dict and
 * the setting "decompress_shared_dict" (no workspace), then the packed entries lz4flex_decompress_batch_packed / lz4flex_compress_batch_packed
 * with lz4flex_packed_work_size, lz4flex_compress_packed_scratch_bound and the read-only setting "packed_scan_tile" (no workspace in the
 * context: the caller brings it), then the dictionary sets lz4flex_dict_set_create / _free / _count with lz4flex_compress_batch_dict_set and
 * lz4flex_decompress_batch_dict_set (no workspace in the context: a set owns its memory), then the partial decode
 * lz4flex_decompress_batch_partial / lz4flex_decompress_partial_into with the setting "decompress_partial" (no workspace), then the
 * seekable frames lz4flex_frame_index_create / _free / _blocks / _content_size / _frame_bytes / _info / _table and
 * lz4flex_frame_read_ranges with the settings "frame_range_pass_bytes" and "frame_range_checksums" (no workspace in the context beyond
 * the scratch the *_many calls already grow: an index owns its tables), then partial decode against dictionaries
 * lz4flex_decompress_batch_partial_shared_dict / lz4flex_decompress_batch_partial_dict_set / lz4flex_decompress_partial_into_with_dict (no
 * new setting, no workspace) -- a caller detects them by the symbol -- then "compress_mode" 2 (high) with the setting "compress_depth" (no
 * new symbol, no workspace beyond the encoder's: a caller detects the mode by lz4flex_set_tuning(ctx, "compress_mode", 2) == 0), then the
 * dictionary trainer lz4flex_dict_train with lz4flex_dict_train_work_size (no setting, no workspace in the context: the caller brings it),
 * then the typed batches lz4flex_filter_batch / lz4flex_compress_batch_typed / lz4flex_decompress_batch_typed with the LZ4FLEX_FILTER_*
 * constants and the setting "filter_bytewise" (no workspace in the context: the caller brings the tmp slots), then the flag
 * LZ4FLEX_FILTER_DELTA (0x10) for the `filter` argument of those three entries, with LZ4FLEX_DELTA_RESTART (no new symbol, no setting: a
 * caller detects it by lz4flex_filter_batch(NULL, ..., n = 0, ..., filter = 0x10, ...) == 0), then the fit batches lz4flex_fit_batch /
 * lz4flex_compress_batch_fit with lz4flex_compress_fit_work_size and the setting "fit_serial" (no workspace in the context: the caller
 * brings scratch and work; a caller detects them by the symbol), then the setting "compress_parse" for "compress_mode" 2 (no new symbol,
 * no workspace beyond the encoder's: a caller detects it by lz4flex_set_tuning(ctx, "compress_parse", 1) == 0), then the paged streams
 * lz4flex_compress_paged with lz4flex_compress_paged_work_size, lz4flex_paged_pages_bound and lz4flex_paged_rounds_bound (no setting, no
 * workspace in the context: the caller brings scratch and work; a caller detects them by the symbol), then their read side
 * lz4flex_paged_read_ranges with lz4flex_paged_read_work_size and lz4flex_paged_range_pages_bound (no setting, no workspace in the
 * context in MEM_DEVICE: the caller brings scratch and work; a caller detects them by the symbol), then the append
 * lz4flex_paged_append with lz4flex_paged_append_work_size and lz4flex_paged_append_stage_bound (no setting, no workspace in the context
 * in MEM_DEVICE: the caller brings stage, scratch and work; a caller detects them by the symbol). */
int lz4flex_abi_version(void);
/* last HIP error string seen by this thread (diagnostics) */
const char *lz4flex_last_error(void);

/* ---- block: scalar, lz4_flex signatures ---------------------------------------------------- */
/* block::get_maximum_output_size, src/block/compress.rs:588-590 */
size_t lz4flex_get_maximum_output_size(size_t input_len);
/* WHAT A SCALAR CALL COSTS.  The lz4_flex-shaped scalar entries below are 1-block batches through the same kernels: one transfer
 * up (descriptors + input from page-locked staging), the kernels, one transfer down, one synchronisation.  Measured on an MI355X
 * (profiles/r06_scalar_latency.txt): a 1 KiB block 0.06 ms either way, a 64 KiB block 0.32 - 0.36 ms to compress and 0.15 ms to
 * decompress (one block occupies one of 256 CUs: the kernel, not PCIe, is the cost), 16 MiB 10 / 25 ms -- a CPU core does a 64 KiB
 * block in 0.04 / 0.012 ms.  These entries exist so that code written against lz4_flex links and runs; the throughput of this
 * library is in the BATCH entries (lz4flex_compress_batch / lz4flex_decompress_batch: thousands of blocks per launch, device-
 * resident buffers) and the frame encoder / decoder, which batch internally.  Batch or lose. */
/* block::compress_into, src/block/compress.rs:599-601.  Err(OutputTooSmall) up front iff
 * out_cap < get_maximum_output_size(in_len) (:338-340).
 * CONTRACT OF THE OUTPUT BYTES (this entry point, compress_prepend_size, compress_into_with_table, lz4flex_compress_batch and
 * the frame encoder): in the DEFAULT compress_mode (0, "fast") the block is a valid LZ4 block with this library's own parse --
 * lz4_flex's decoder (and any other LZ4 decoder) returns the input, the ratio is within a percent of lz4_flex's (usually
 * better) -- but the bytes are NOT lz4_flex's.  Callers that hash, deduplicate or golden-file compressed output must select
 * compress_mode 1 ("exact": lz4flex_set_tuning / LZ4FLEX_COMPRESS_MODE=exact), which reproduces the reference encoder byte
 * for byte as restated by oracle/ (no Rust toolchain exists here: "oracle-exact, reference byte-unpinned"). */
int64_t lz4flex_compress_into(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap);
/* block::compress_into_with_dict, src/block/compress.rs:610-616 */
int64_t lz4flex_compress_into_with_dict(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap,
                                        const uint8_t *dict, size_t dict_len);
/* block::compress_prepend_size, src/block/compress.rs:673-675 (LE u32 length prefix) */
int64_t lz4flex_compress_prepend_size(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap);
/* block::compress_prepend_size_with_dict, src/block/compress.rs:692-694 (dictionaries of <= 3 bytes are ignored, :626-628) */
int64_t lz4flex_compress_prepend_size_with_dict(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap,
                                                const uint8_t *dict, size_t dict_len);
/* block::CompressTable + compress_into_with_table, src/block/compress.rs:710-766.  The reference clears the table on every
 * call; the handle avoids re-allocating it and carries its variant: Small (u16 entries, 4-byte hash: what compress_into
 * uses below 65 535 bytes) or Large (u32 entries, 5-byte hash).  An input of >= 65 535 bytes upgrades a Small table to
 * Large for good (:752-754), which changes the bytes later small inputs compress to -- reproduced here.  The handle owns
 * the device workspace reused across calls. */
typedef struct lz4flex_compress_table lz4flex_compress_table;
lz4flex_compress_table *lz4flex_compress_table_new(int large /* 0 = CompressTable::small() / default, 1 = large() */);
void lz4flex_compress_table_free(lz4flex_compress_table *t);
int lz4flex_compress_table_is_large(const lz4flex_compress_table *t);
int64_t lz4flex_compress_into_with_table(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap,
                                         lz4flex_compress_table *table);
/* block::decompress_into, src/block/decompress.rs:454-456 */
int64_t lz4flex_decompress_into(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap,
                                lz4flex_err_detail *detail /* nullable */);
/* block::decompress_into_with_dict, src/block/decompress.rs:462-468 */
int64_t lz4flex_decompress_into_with_dict(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap,
                                          const uint8_t *dict, size_t dict_len, lz4flex_err_detail *detail);
/* The first min(size, target) bytes of one block: a one-block host batch of lz4flex_decompress_batch_partial (its contract, below).
 * Returns the bytes written or -code; there is no OutputTooSmall, so of `detail` only hip_error can be set. */
int64_t lz4flex_decompress_partial_into(const uint8_t *in, size_t in_len, uint8_t *out, size_t target,
                                        lz4flex_err_detail *detail /* nullable */);
/* The same against an external dictionary: a one-block host batch of lz4flex_decompress_batch_partial_shared_dict (its contract, below;
 * dict == NULL or dict_len == 0: lz4flex_decompress_partial_into).  Returns the bytes written or -code (-LZ4FLEX_E_INVALID_ARG: a length
 * beyond 32 bits, dict == NULL with dict_len != 0); of `detail` only hip_error can be set. */
int64_t lz4flex_decompress_partial_into_with_dict(const uint8_t *in, size_t in_len, uint8_t *out, size_t target,
                                                  const uint8_t *dict, size_t dict_len, lz4flex_err_detail *detail /* nullable */);
/* block::uncompressed_size, src/block/mod.rs:151-157: returns the LE u32 prefix or -EXPECTED_ANOTHER_BYTE */
int64_t lz4flex_uncompressed_size(const uint8_t *in, size_t in_len);
/* block::decompress_size_prepended, src/block/decompress.rs:493-496; out_cap must be >= the prefix */
int64_t lz4flex_decompress_size_prepended(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap,
                                          lz4flex_err_detail *detail);

/* block::decompress_size_prepended_with_dict, src/block/decompress.rs:521-527 */
int64_t lz4flex_decompress_size_prepended_with_dict(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap,
                                                    const uint8_t *dict, size_t dict_len, lz4flex_err_detail *detail);

/* ---- block: batched (the hot entry; the frame layer's per-block calls
 *      src/frame/compress.rs:282-298 and src/frame/decompress.rs:288-305, batched) ------------ */
#define LZ4FLEX_MEM_HOST 0   /* every pointer is host memory; the call stages through the ctx arena and is synchronous */
#define LZ4FLEX_MEM_DEVICE 1 /* every pointer (data AND descriptor/result arrays) is device memory; asynchronous on `stream` */
/* OR into mem_kind for DEVICE batches that may hold blocks > 64 KiB: the lengths live in device memory where the host cannot see
 * them (HOST batches detect it themselves).  compress, reference-exact mode: selects the u32 hash table; decompress: a hint
 * that the blocks are large, so any number of them goes to the one-workgroup-per-block decoder (lz4_decompress_pcd.hip), which
 * otherwise serves batches of up to 1 024 blocks.  Results do not depend on the hint. */
#define LZ4FLEX_MEM_BIG_BLOCKS 0x100

/* OR into mem_kind for lz4flex_decompress_batch_ex with ext->out_pos: the batch is a CHAIN -- every block has the same out_off,
 * and block i's prefix [out_off, out_off + out_pos[i]) is what blocks 0 .. i-1 of this batch produce (plus whatever lay before
 * out_pos[0] when the call was made).  This is how a Linked frame's blocks are decoded in one launch
 * (src/frame/decompress.rs:195-222,280-306: the reference decodes them one after the other into one window): the token chains
 * of all blocks are parsed at once, a block waits for its predecessors only where a match really reaches behind its start.
 * At most 65 536 blocks per call; no external dictionaries. */
#define LZ4FLEX_MEM_CHAINED 0x200

/* per-block compress flags.  They select among the REFERENCE's hash tables and therefore only have a meaning in compress_mode
 * exact; the throughput encoder (compress_mode fast, the default) has one table layout of its own and ignores them, as it
 * ignores the Small / Large state of a lz4flex_compress_table. */
#define LZ4FLEX_BLOCK_DEFAULT 0u            /* block::compress_into: table/hash picked by length (compress.rs:559-566) */
/* bit 1: the FrameEncoder's table (HashTable4K + 5-byte hash whatever the length,
 * src/frame/compress.rs:76,141) with a freshly zeroed table: block 0 of a frame */
#define LZ4FLEX_BLOCK_FRAME_FIRST 2u
/* bits 1|0: block k>0 of an Independent frame: same table, every entry unreachable, position 0
 * is probed (src/frame/compress.rs:357-367, src/block/compress.rs:353-359,422-429) */
#define LZ4FLEX_BLOCK_FRAME_CONTINUATION 3u
/* bits 8..31, any compress_mode's flag word: h bytes of the SAME STREAM lie in front of the block, readable at
 * in_base[in_off[i] - h .. in_off[i]) -- block k > 0 of a Linked frame (src/frame/compress.rs:280-299,327-356: the reference
 * keeps the previous 64 KiB of input as the next block's dictionary).  The throughput encoder then lets the block's matches
 * reach into them: with h >= 32 768 every position sees between 32 and 64 KiB of the stream behind it (a smaller h is not
 * used), all blocks of the batch still encode side by side, and the block can only be decoded behind those bytes (a Linked
 * frame, LZ4FLEX_MEM_CHAINED, or lz4flex_decompress_batch_ex with them as out_pos prefix / dictionary).  compress_mode exact
 * ignores the bits: the reference's bytes for dependent blocks come from lz4flex_compress_chains.  compress_mode high ignores them
 * too by default: a raw lz4flex_compress_batch block is encoded as an independent block, which is valid behind any history (the
 * frame layer writes its Linked frames with the throughput encoder in that mode).  With "compress_high_linked" 1 it reads them: the
 * last min(h, 32 768) bytes in front of the block are searched as deeply as the block itself (h < 4: none), see that setting. */
#define LZ4FLEX_BLOCK_HISTORY(h) ((uint32_t)(h) << 8)

/* Compress n independent blocks.  Block i reads in_base[in_off[i] .. +in_len[i]] and writes at
 * out_base[out_off[i] ..], capacity out_cap[i] (must be >= get_maximum_output_size(in_len[i]),
 * else status[i] = LZ4FLEX_E_OUTPUT_TOO_SMALL and nothing is written).  out_len[i] = bytes
 * written.  flags may be NULL.  hip_stream: the hipStream_t a MEM_DEVICE batch is enqueued on (NULL = HIP's
 * null stream); MEM_HOST batches ignore it and use the context's own stream.
 * Returns 0 or -code for call-level failures; per-block results are in status[]. */
int lz4flex_compress_batch(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                           const uint32_t *flags, uint32_t n, void *out_base, const uint64_t *out_off,
                           const uint32_t *out_cap, uint32_t *out_len, int32_t *status, int mem_kind,
                           void *hip_stream);

/* Compress n independent blocks, each against an external dictionary of its own: block::compress_into_with_dict
 * (src/block/compress.rs:554-616) as a batch.  Block i reads in_base[in_off[i] .. + in_len[i]], its dictionary is
 * dict_base[dict_off[i] .. + dict_len[i]] (dict_len[i] == 0: none); dictionaries may overlap each other and the inputs.
 * Everything not said here is as for lz4flex_compress_batch (the OUTPUT_TOO_SMALL rule; MEM_HOST: staged -- the dictionary
 * spans travel with the batch -- and synchronous; MEM_DEVICE: every pointer, the ext arrays included, is device memory, the call
 * is asynchronous on hip_stream and allocates nothing).
 *   No dictionaries: ext == NULL, ext->dict_base == NULL, or every dict_len[i] == 0 behaves as lz4flex_compress_batch and gives
 *     the same bytes; a block with dict_len[i] == 0 in a mixed batch gets the bytes lz4flex_compress_batch gives it in a batch of
 *     the same size.
 *   compress_mode exact: block i gets exactly the bytes of lz4flex_compress_into_with_dict(block, dict) -- the table kind from the
 *     UNtruncated dict_len + in_len < 65 535 (compress.rs:559), init_dict over the dictionary's last 64 KiB, every third position
 *     (:571-583); dictionaries of 1 - 3 bytes count (only the _prepend_size_ helpers ignore them, :626-628).  One-block chains
 *     of the reference-exact chain encoder (lz4flex_compress_chains), their records built on the device.
 *   compress_mode fast (the default): block i is encoded by the throughput encoder as the item [last h bytes of the dictionary |
 *     block], h = min(dict_len[i], 32 768): the LZ4FLEX_BLOCK_HISTORY mechanism with the history read from the dictionary; no
 *     sub-windows.  The bytes depend only on the block, the dictionary's last h bytes and "compress_sliding_window" -- never on
 *     the batch or the device -- and they decode with decompress_into_with_dict(block, dict) or any dictionary that ends in the
 *     same h bytes.  Measured on an MI355X (profiles/r08_dict_compress.txt; one 32 KiB
 *     dictionary, device-resident batches): 16 384 x 64 KiB JSON tiles 5.5 ms (3.0 without a dictionary, 67 ms in exact mode),
 *     ratio 0.200 (0.230; exact 0.163); 65 536 x 4 KiB log records 5.8 ms (6.2 without, 58 in exact mode), ratio 0.298 (0.391;
 *     exact 0.315) -- fast mode is the faster one for both shapes, even though a 4 KiB record indexes 32 KiB of dictionary.
 *   Refused: a block with a dictionary and flags[i] != 0 (frame tables, LZ4FLEX_BLOCK_HISTORY and a dictionary do not combine)
 *     gets status LZ4FLEX_E_INVALID_ARG, out_len 0, and nothing is written; the other blocks of the batch are unaffected.
 * Returns 0 or -code for call-level failures (-LZ4FLEX_E_INVALID_ARG: dict_base set and dict_off / dict_len NULL). */
typedef struct lz4flex_compress_ext {
    const void *dict_base;      /* same memory kind as the batch; NULL = no dictionaries */
    const uint64_t *dict_off;
    const uint32_t *dict_len;   /* 0 = this block has no dictionary */
} lz4flex_compress_ext;
int lz4flex_compress_batch_ex(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                              const uint32_t *flags, uint32_t n, void *out_base, const uint64_t *out_off,
                              const uint32_t *out_cap, uint32_t *out_len, int32_t *status,
                              const lz4flex_compress_ext *ext, int mem_kind, void *hip_stream);

/* Compress n independent blocks against ONE dictionary: the many-small-records use of lz4flex_compress_batch_ex, with the work
 * that depends on the dictionary alone done once per call instead of once per block.  `dict` (dict_len bytes, a HOST value in both
 * memory kinds) lies in the same memory kind as the batch.  There are no flags: dictionaries and flags do not combine.
 * Everything not said here is as for lz4flex_compress_batch_ex (the OUTPUT_TOO_SMALL rule, LZ4FLEX_MEM_BIG_BLOCKS; MEM_HOST: staged and
 * synchronous; MEM_DEVICE: asynchronous on hip_stream, allocates nothing).
 *   The bytes: block i gets exactly what lz4flex_compress_batch_ex gives it with dict_off[i] = 0, dict_len[i] = dict_len for every
 *     i, in both compress modes and under every "compress_sliding_window".  dict == NULL or dict_len == 0: lz4flex_compress_batch
 *     without flags.
 *   compress_mode fast: an item is [last h bytes of the dictionary | block], h = min(dict_len, 32 768), and what the encoder's
 *     indexer does to its first hs positions -- hs = the largest multiple of 1 024 with hs + 3 <= h -- is the same for every item.  A
 *     small kernel in front of the encoder does it once (the digest: the hash table after those positions, whether they are one
 *     byte repeated, the tail itself; it lives in the context's workspace); the first window of every item whose positions below
 *     hs may all start a match (block length >= hs + 11 - h) loads that table instead of clearing it, indexes from hs on, and stages
 *     only the block behind the tail its workgroup's staging slot already holds.  Every other item (a dictionary shorter than
 *     1 027 bytes, a block of a few bytes, the later windows of a block longer than 32 KiB) takes the per-block path in the same kernel.
 *     Setting "compress_shared_dict" (default 1): 0 = no item starts from the digest (the per-block path for all of them: A/B
 *     measurements, tests).  Measured on an MI355X (profiles/r09_shared_dict.txt; one 32 KiB dictionary, device-resident batches,
 *     this entry against lz4flex_compress_batch_ex alternating in one session): 65 536 x 4 KiB log records 5.47 ms against 5.67 ms
 *     (1.04 x), 16 384 x 64 KiB JSON tiles 5.01 ms against 5.52 ms (1.10 x).  The indexer's work per 4 KiB record falls 3.5 x, but it
 *     runs beside the workers, and a record's window waits for the one worker that parses 3 of its 4 KiB (the segment geometry is
 *     part of the bytes).
 *   compress_mode exact: the one-block chains of lz4flex_compress_batch_ex with the one dictionary.
 * Returns 0 or -code for call-level failures (-LZ4FLEX_E_INVALID_ARG: a missing array, dict == NULL with dict_len != 0, a mem_kind
 * other than HOST / DEVICE (| BIG_BLOCKS)); n == 0 returns 0. */
int lz4flex_compress_batch_shared_dict(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                                       uint32_t n, void *out_base, const uint64_t *out_off, const uint32_t *out_cap,
                                       uint32_t *out_len, int32_t *status, const void *dict, uint32_t dict_len,
                                       int mem_kind, void *hip_stream);

/* Chains of DEPENDENT blocks: the full compress_internal signature (src/block/compress.rs:289-325) -- a
 * prefix before in_pos, an external dictionary, a stream offset and ONE hash table that persists across
 * the blocks of a chain (Linked frames, src/frame/compress.rs:280-299,327-356; compress_into_with_dict,
 * :554-583).  Chains run in parallel, the blocks of a chain in order.  All offsets index in_base. */
typedef struct lz4flex_chain_block {
    uint64_t in_off;    /* start of `input` (prefix included) */
    uint64_t dict_off;  /* start of ext_dict */
    uint32_t in_len;    /* input.len() */
    uint32_t in_pos;    /* input_pos: first byte to compress */
    uint32_t dict_len;
    uint32_t so;        /* input_stream_offset */
    uint32_t repos;     /* HashTable4K::reposition(repos) before this block (hashtable.rs:113-117); 0 = none */
    uint32_t flags;     /* bit0: 4-byte hash (the HashTable4KU16 case of compress.rs:559-562); bit1: clear the table and init_dict (:571-583) */
} lz4flex_chain_block;
/* blocks[chain_first[c] .. +chain_count[c]) form chain c; out_off/out_cap/out_len/status are per block.
 * tbl_state (nullable): 4096 u32 per chain, read before the chain's first block and written back after its
 * last one, so a chain can continue in a later call.  MEM_HOST or MEM_DEVICE as for the batches. */
int lz4flex_compress_chains(lz4flex_ctx *ctx, const void *in_base, const lz4flex_chain_block *blocks, uint32_t n_blocks,
                            const uint32_t *chain_first, const uint32_t *chain_count, uint32_t n_chains,
                            void *out_base, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len,
                            int32_t *status, uint32_t *tbl_state, int mem_kind, void *hip_stream);

/* Decompress n independent blocks.  out_cap[i] >= true size (larger allowed, as
 * decompress_into).  status[i] = 0 or a DecompressError code; detail (nullable, 2*n u64:
 * expected, actual) is filled for OutputTooSmall. */
int lz4flex_decompress_batch(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                             uint32_t n, void *out_base, const uint64_t *out_off, const uint32_t *out_cap,
                             uint32_t *out_len, int32_t *status, uint64_t *detail, int mem_kind,
                             void *hip_stream);

/* The decompressed sizes of n raw blocks (no size prefix, no frame): what block::decompress_into (src/block/decompress.rs:201-449)
 * would return for block i = in_base[in_off[i] .. + in_len[i]) with a sink too large for OutputTooSmall and history[i] bytes in front
 * of the block's output (the ext_dict_len of decompress_into_with_dict, or the out_pos of lz4flex_decompress_batch_ex's prefix form:
 * it only decides the OffsetOutOfBounds check, :399-401; history NULL = 0).  out_size[i] = the NEW bytes the block produces, prefix not
 * counted (u64: a block expands up to 255 x), status[i] = 0 or the first error in the reference's check order (LITERAL_OUT_OF_BOUNDS,
 * EXPECTED_ANOTHER_BYTE -- the empty block too, :207-209 -- OFFSET_ZERO, OFFSET_OUT_OF_BOUNDS); out_size[i] = 0 when status[i] != 0.
 * Nothing is decoded and nothing but out_size / status is written.  A block with status 0 and size S decodes with out_cap = S (and the
 * same history) on every decoder configuration, to out_len S.  So a caller that holds raw blocks without their sizes runs this, an
 * exclusive prefix sum of out_size for the out_off, and one lz4flex_decompress_batch with out_cap = out_size -- all of it on the device.
 * mem_kind: LZ4FLEX_MEM_HOST (staged through the context, synchronous) or LZ4FLEX_MEM_DEVICE (every pointer device memory, asynchronous
 * on hip_stream); LZ4FLEX_MEM_BIG_BLOCKS may be ORed in (a hint, results do not depend on it).  n == 0 returns 0.  Returns 0 or -code.
 * Setting "size_scan_serial" (tests): 1 = every block is measured by the serial pass alone (lz4_size_scan.hip), 0 (default). */
int lz4flex_decompressed_size_batch(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                                    uint32_t n, const uint32_t *history, uint64_t *out_size, int32_t *status, int mem_kind,
                                    void *hip_stream);

/* ---- packed batches: ONE output buffer, the offsets computed on the device -------------------------------------------------
 * The batched entries above take the output layout from the caller (out_off[], out_cap[]).  A caller that holds n size-prepended
 * blocks (block::compress_prepend_size's output), or raw blocks, cannot know that layout before the sizes are known; a caller that
 * compresses wants the produced bytes back to back with an offset table, not one worst-case slot per block.  The two entries below
 * take ONE buffer of total_cap bytes and write the layout themselves: out_off[0 .. n] = the exclusive prefix sums of the slot sizes,
 * each rounded up to `align` (a power of two from 1 to 256; 1 = dense), out_off[n] = the bytes the batch needs.
 *   The fit rule: block i fits iff out_off[i] + size[i] <= total_cap.  A block that does not fit gets status LZ4FLEX_E_OUTPUT_TOO_SMALL,
 *     out_len 0, capacity 0 and (decode) detail {expected = out_off[i] + size[i], actual = total_cap}; nothing of it is written.  It is
 *     applied to every block, also to one whose size is 0 or unknown.  out_off[] is the pure scan in every case: out_off[n] is the
 *     capacity the batch needs even when it exceeds total_cap, so a caller can enlarge the buffer and call again.
 *   total_cap and align are HOST values.  mem_kind: LZ4FLEX_MEM_DEVICE -- every pointer is device memory, `work` holds
 *     lz4flex_packed_work_size(n) bytes (8-byte aligned), the call is asynchronous on hip_stream, allocates nothing, copies nothing to
 *     the host and never synchronises -- or LZ4FLEX_MEM_HOST -- staged through the context and synchronous; `work` and `scratch` are
 *     ignored.  LZ4FLEX_MEM_BIG_BLOCKS may be ORed in; LZ4FLEX_MEM_CHAINED is refused.  No dictionaries.
 *   The arguments are checked before a context or a device is looked at: -LZ4FLEX_E_INVALID_ARG for an unknown size_mode, an align that
 *     is not a power of two from 1 to 256, a mem_kind other than HOST / DEVICE (| BIG_BLOCKS), and -- n != 0 -- a missing array,
 *     sizes == NULL in GIVEN mode, work == NULL (compress: or scratch == NULL) in a DEVICE call.  n == 0 returns 0.
 *   The kernels (lz4_packed.hip): the sizes, an exclusive scan in three phases (every workgroup sums a tile of "packed_scan_tile" sizes
 *     -- a read-only setting --, one workgroup scans the tile sums, every workgroup scans its tile; integer sums in a fixed order), and
 *     on the compress side a gather, one workgroup per block, 16 bytes per lane where source and destination allow.
 *   Not timed: tools/packed_bench.py times both entries against the plain batch calls and against block.decompress_blocks_device
 *     (profiles/r11_packed.txt awaits the table). */
#define LZ4FLEX_SIZES_PREPENDED 0   /* block::decompress_size_prepended, src/block/decompress.rs:493-499 */
#define LZ4FLEX_SIZES_GIVEN     1   /* block::decompress(input, min_uncompressed_size), :508-517 */
#define LZ4FLEX_SIZES_SCAN      2   /* raw blocks, sizes by lz4flex_decompressed_size_batch */

/* bytes of `work` a MEM_DEVICE call of either packed entry needs for n blocks */
size_t lz4flex_packed_work_size(uint32_t n);
/* bytes of `scratch` that hold the slots of lz4flex_compress_batch_packed for ANY n blocks of total_in_bytes bytes together: at least
 * the sum of get_maximum_output_size(in_len[i]) + (prepend_size ? 4 : 0) */
uint64_t lz4flex_compress_packed_scratch_bound(uint64_t total_in_bytes, uint32_t n, int prepend_size);

/* Decompress n independent blocks into one buffer, slot after slot.  The slot size of block i:
 *   LZ4FLEX_SIZES_PREPENDED: the LE u32 in front of the block (in_base[in_off[i] .. + 4), any alignment); the block proper is the
 *     in_len[i] - 4 bytes behind it.  in_len[i] < 4: size 0 and status LZ4FLEX_E_EXPECTED_ANOTHER_BYTE (block::uncompressed_size,
 *     src/block/mod.rs:151-157).  out_len may be smaller than the prefix (the reference truncates its Vec); the slot keeps the prefix's
 *     size.  A hostile prefix does not fit and gets OUTPUT_TOO_SMALL -- the reference would allocate it.
 *   LZ4FLEX_SIZES_GIVEN: sizes[i], the min_uncompressed_size of block::decompress.
 *   LZ4FLEX_SIZES_SCAN: what lz4flex_decompressed_size_batch measures (history 0).  A block the size pass rejects keeps that status
 *     and gets an empty slot; a block of more than 4 GiB - 1 bytes gets size 0 and status LZ4FLEX_E_UNSUPPORTED.
 * Written: out_off (n + 1), out_cap (n: the slot sizes, 0 for a block without room), out_len, status, detail (nullable, 2 n: every
 * entry is written, {0, 0} for a block whose status is not OUTPUT_TOO_SMALL).
 * A block that fits gets exactly what lz4flex_decompress_batch gives it with out_off[i] and out_cap[i] = its slot size: bytes, out_len,
 * every DecompressError variant, and the OutputTooSmall detail counted from the slot.  Nothing is written outside
 * [out_off[i], out_off[i] + out_len[i]) of fitting blocks, and nothing beyond total_cap. */
int lz4flex_decompress_batch_packed(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                                    uint32_t n, int size_mode, const uint32_t *sizes /* GIVEN only */, void *out_base,
                                    uint64_t total_cap, uint32_t align, uint64_t *out_off /* n + 1, written */,
                                    uint32_t *out_cap /* n, written: the slot sizes */, uint32_t *out_len, int32_t *status,
                                    uint64_t *detail /* nullable */, void *work, int mem_kind, void *hip_stream);

/* Compress n independent blocks into one packed stream.  The encoder writes block i into a slot of get_maximum_output_size(in_len[i])
 * (+ 4 with prepend_size) bytes of `scratch`, slot behind slot; the produced lengths are scanned into out_off and the payloads copied
 * to out_base + out_off[i].  The payload of block i is, byte for byte, what lz4flex_compress_batch (flags NULL) gives the same batch
 * under the same settings.  prepend_size != 0: the payload follows the LE u32 in_len[i] and out_len[i] counts the 4 -- under
 * compress_mode exact the reference's compress_prepend_size output (src/block/compress.rs:673-675), what LZ4FLEX_SIZES_PREPENDED reads.
 * A block the encoder refuses keeps its status and takes no room in the stream (out_len 0).
 * scratch_cap: MEM_HOST (the lengths are visible) -LZ4FLEX_E_INVALID_ARG when it is below the sum of the slots; MEM_DEVICE: the fit rule
 * on the scratch slots -- a block whose slot ends behind scratch_cap gets OUTPUT_TOO_SMALL, the others are unaffected.
 * lz4flex_compress_packed_scratch_bound gives a capacity that always holds.
 * Written: out_off (n + 1), out_len, status. */
int lz4flex_compress_batch_packed(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                                  uint32_t n, int prepend_size, void *scratch, uint64_t scratch_cap, void *out_base,
                                  uint64_t total_cap, uint32_t align, uint64_t *out_off /* n + 1, written */, uint32_t *out_len,
                                  int32_t *status, void *work, int mem_kind, void *hip_stream);

/* Optional per-block extras for decoding: an external dictionary (block::decompress_into_with_dict,
 * src/block/decompress.rs:462-468) and/or an initial sink position: the output region
 * [out_off, out_off+out_pos) already holds earlier bytes that matches may reference (the prefix mode
 * of Linked frames, src/frame/decompress.rs:293-306); out_len counts only the new bytes.  out_pos[i] <= out_cap[i] is required
 * (out_cap counts from out_off, prefix included; out_pos == out_cap is legal and leaves room for an empty block only): a block
 * with out_pos[i] > out_cap[i] gets status LZ4FLEX_E_INVALID_ARG, out_len 0 and detail 0, and nothing is written (the reference
 * panics there, src/sink.rs:103-107); in a CHAINED batch it ends its chain as a decode error does.  The OutputTooSmall detail
 * counts from out_off too, prefix included (src/block/decompress.rs:349-355,402-407): {expected, actual = out_cap}. */
typedef struct lz4flex_decompress_ext {
    const void *dict_base;     /* nullable */
    const uint64_t *dict_off;
    const uint32_t *dict_len;
    const uint32_t *out_pos;   /* nullable */
    /* nullable; LZ4FLEX_MEM_DEVICE | LZ4FLEX_MEM_CHAINED batches only: the batch holds SEVERAL chains (N Linked frames decoded side
     * by side, lz4flex_frame_decompress_many).  Block i's predecessor in its chain is block chain_prev[i] -- an index BELOW i -- or
     * 0xFFFFFFFF for the first block of a chain; the blocks of one chain share an out_off, different chains have regions of their
     * own.  Order the blocks level by level (every chain's block k before any chain's block k + 1) and all chains advance together. */
    const uint32_t *chain_prev;
    uint32_t n_chains;         /* with chain_prev: how many chains the batch holds (a hint for the kernel geometry: few chains get a
                                * large workgroup per block, many chains small ones); 0 = unknown */
} lz4flex_decompress_ext;
int lz4flex_decompress_batch_ex(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                                uint32_t n, void *out_base, const uint64_t *out_off, const uint32_t *out_cap,
                                uint32_t *out_len, int32_t *status, uint64_t *detail,
                                const lz4flex_decompress_ext *ext, int mem_kind, void *hip_stream);

/* Decompress n independent blocks against ONE dictionary: the mirror of lz4flex_compress_batch_shared_dict.  `dict` (dict_len bytes, a
 * HOST value in both memory kinds) lies in the same memory kind as the batch.  mem_kind: LZ4FLEX_MEM_HOST (staged, the dictionary once
 * per call; synchronous) or LZ4FLEX_MEM_DEVICE (asynchronous on hip_stream, allocates nothing); LZ4FLEX_MEM_BIG_BLOCKS may be ORed in
 * (results do not depend on it); LZ4FLEX_MEM_CHAINED is refused.
 *   The results: block i gets exactly what lz4flex_decompress_batch_ex gives it with dict_base = dict, dict_off[i] = 0, dict_len[i] =
 *     dict_len and no out_pos -- bytes, out_len, status (every DecompressError in the reference's check order; OffsetOutOfBounds is
 *     offset > produced + dict_len, src/block/decompress.rs:399-401) and detail (OutputTooSmall {expected, actual = out_cap}, counted from
 *     out_off).  Nothing is written behind out_len bytes of a sink, nothing in front of out_off, never into the dictionary.  dict == NULL
 *     or dict_len == 0: lz4flex_decompress_batch.
 *   The kernel: lz4flex_decompress_batch_ex decodes dictionary blocks sixteen lanes per block, a block's sequences one after the other
 *     (lz4_decompress.hip).  This entry runs the sequence decoder (lz4_decompress_seq.hip: a wavefront per block, a lane per sequence) in
 *     its dictionary form at every n: the dictionary's last min(dict_len, 65 536) bytes are a virtual prefix in front of every block's
 *     output, read from the one buffer and never stored to; a match that starts in the dictionary and ends in the block is decoded there.
 *     Blocks it cannot decode (errors, sinks too small) are decoded again in the reference's order with the dictionary.
 *     Setting "decompress_shared_dict" (default 1): 0 = every block in the reference's order, sixteen lanes per block (the per-block
 *     path's decode_block; A/B measurements, tests); "decompress_variant" 1 pinned has the same effect.
 *     Not timed yet: tools/shared_dict_decode_bench.py times this entry against lz4flex_decompress_batch_ex with per-block arrays and
 *     against the same records without a dictionary (profiles/r10_shared_dict_decode.txt holds the register figures and awaits the table).
 * Returns 0 or -code for call-level failures (-LZ4FLEX_E_INVALID_ARG: a missing array, dict == NULL with dict_len != 0, a mem_kind
 * other than HOST / DEVICE (| BIG_BLOCKS)); n == 0 returns 0. */
int lz4flex_decompress_batch_shared_dict(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                                         uint32_t n, void *out_base, const uint64_t *out_off, const uint32_t *out_cap,
                                         uint32_t *out_len, int32_t *status, uint64_t *detail /* nullable */,
                                         const void *dict, uint32_t dict_len, int mem_kind, void *hip_stream);

/* PARTIAL DECODE: the first target[i] bytes of every block of a batch (a record header, the first rows of a page, a format sniff over
 * thousands of stored blocks) -- C liblz4's LZ4_decompress_safe_partial as a batch; its cost is that of the bytes asked for, not of the
 * block.  mem_kind: LZ4FLEX_MEM_HOST (staged, synchronous; the output staging is sized from target[], not from the blocks) or
 * LZ4FLEX_MEM_DEVICE (every pointer device memory, asynchronous on hip_stream, allocates nothing); LZ4FLEX_MEM_BIG_BLOCKS may be ORed in
 * (a hint: results do not depend on it); LZ4FLEX_MEM_CHAINED is refused.  No dictionaries, no out_pos prefixes, no chains.
 *   The contract, for block i of n = in_len[i] bytes and target = target[i] (lines: src/block/decompress.rs):
 *       if n == 0: ExpectedAnotherByte                                     (:207-209, before anything else)
 *       op = 0
 *       while op < target:
 *           token; literal length with all its length bytes                 (ExpectedAnotherByte if the input ends inside them)
 *           if lit > n - ip: LiteralOutOfBounds                             (the FULL length is checked, in the reference's order)
 *           copy min(lit, target - op) literals; op += that; ip += lit
 *           if op == target: stop, status 0
 *           if ip >= n: stop, status 0                                      (the block's normal end, :366-368)
 *           if n - ip < 2: ExpectedAnotherByte
 *           offset; if 0: OffsetZero
 *           match length with all its length bytes                          (ExpectedAnotherByte if the input ends inside them)
 *           if offset > op: OffsetOutOfBounds
 *           copy min(ml, target - op) match bytes (byte-serial forward semantics, overlap included); op += that
 *           if op == target: stop, status 0                                 (the "a match is followed by a token" check is NOT made here)
 *           if ip >= n: ExpectedAnotherByte                                 (:439-443)
 *       out_len = op, status 0
 *   - A valid block of size S: out_len = min(S, target), the bytes are the first out_len bytes lz4flex_decompress_batch produces, status
 *     0.  target >= S behaves as lz4flex_decompress_batch with out_cap = target.
 *   - There is no LZ4FLEX_E_OUTPUT_TOO_SMALL and no detail array: target is a wish, not a capacity that can be violated.
 *   - An error the reference would meet before target bytes exist is reported, in the reference's order; an error behind that point is
 *     not seen.  target == 0 on a non-empty block: status 0, out_len 0, nothing is read.
 *   - On error out_len is 0 and the target bytes of the sink may hold anything.
 *   - Nothing is ever written at or behind out_off[i] + target[i], nothing in front of out_off[i].  This is strict: the sink ends at target.
 *   The kernels: the sequence decoder (lz4_decompress_seq.hip: a wavefront per block, a lane per sequence) in its partial form at every n:
 *     a chunk of sequences is cut in front of the one that reaches or crosses the target, that one is executed alone by the wavefront,
 *     clipped, and the block's tile loop ends there -- no tile of 3 840 compressed bytes behind the one that holds the stop is staged or
 *     walked.  Blocks it hands back (an empty block, more than 4 GiB - 64 KiB of input, errors in front of the stop, an irregular
 *     token list -- also one whose irregularity lies behind the stop, inside the stop's tile) are decoded again in the reference's order,
 *     sixteen lanes per block, up to their target (lz4_decompress.hip lz4_decompress_partial_kernel: the definition above, literally).
 *     Setting "decompress_partial" (default 1): 0 = every block in the reference's order, sixteen lanes per block (A/B measurements,
 *     tests); "decompress_variant" 1 pinned has the same effect.  "decompress_second_pass" 0 leaves handed-back blocks marked 0x7F000001.
 *     Measured on an MI355X (tools/partial_bench.py, one session, profiles/r13_partial.txt; 64 KiB JSON tiles, device-resident, ms per
 *     call for 4 096 / 16 384 blocks): a full decode 0.48 / 1.66; this entry at target 64: 0.056 / 0.143, at 4 096: 0.082 / 0.232, at
 *     65 536: 0.49 / 1.74 (level with the plain sequence decoder, 0.49 / 1.74).  "decompress_partial" 0 at the same targets: 0.010 /
 *     0.011, 0.47 / 0.65, 5.9 / 8.5 -- the reference's order wins where the target is a few dozen bytes (the sequence decoder stages and
 *     walks one whole tile of 3 840 compressed bytes whatever the target) and loses from a few KiB on.
 * Returns 0 or -code for call-level failures (-LZ4FLEX_E_INVALID_ARG: a missing array, a mem_kind other than HOST / DEVICE
 * (| BIG_BLOCKS); the arguments are checked before a context is looked at); n == 0 returns 0; -LZ4FLEX_E_NO_DEVICE without a device. */
int lz4flex_decompress_batch_partial(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                                     uint32_t n, void *out_base, const uint64_t *out_off, const uint32_t *target,
                                     uint32_t *out_len, int32_t *status, int mem_kind, void *hip_stream);

/* PARTIAL DECODE AGAINST A DICTIONARY: the first target[i] bytes of every block of a batch whose blocks were compressed against ONE
 * dictionary (lz4flex_compress_batch_shared_dict) -- a record's header or key prefix out of tens of thousands of small records, without
 * decoding any of them in full.  `dict` (dict_len bytes, a HOST value in both memory kinds) lies in the same memory kind as the batch.
 * mem_kind: LZ4FLEX_MEM_HOST (staged, synchronous: the batch, the output staging sized from target[], the dictionary once per call) or
 * LZ4FLEX_MEM_DEVICE (asynchronous on hip_stream, allocates nothing); LZ4FLEX_MEM_BIG_BLOCKS may be ORed in (results do not depend on it);
 * LZ4FLEX_MEM_CHAINED is refused.  No per-block dictionary arrays, no out_pos prefixes, no chains.
 *   The contract is lz4flex_decompress_batch_partial's, with one line changed:
 *           if offset > op + dict_len: OffsetOutOfBounds                    (dict_len untruncated, src/block/decompress.rs:399-401)
 *     and the bytes of a match whose source lies in front of the output come from the dictionary's end (copy_from_dict, :85-109 /
 *     :410-426), clipped to the target like every other copy.  Everything else carries over: out_len = min(S, target); no
 *     LZ4FLEX_E_OUTPUT_TOO_SMALL and no detail array; errors in front of the target in the reference's order, errors behind it not seen;
 *     target == 0 on a non-empty block: status 0, out_len 0, nothing is read; an empty block: LZ4FLEX_E_EXPECTED_ANOTHER_BYTE; on error
 *     out_len is 0.  Strict: nothing is written at or behind out_off[i] + target[i], nothing in front of out_off[i], and nothing is ever
 *     written into the dictionary.
 *   Equalities: a target at or beyond a valid block's size gives the results of lz4flex_decompress_batch_shared_dict with out_cap =
 *     target.  dict == NULL or dict_len == 0: the call is forwarded to lz4flex_decompress_batch_partial.  The results are those of
 *     lz4flex_decompress_batch_partial_dict_set with a set of this one dictionary.
 *   The kernels: the sequence decoder (lz4_decompress_seq.hip) in its form with both a dictionary and a target -- the dictionary's last
 *     min(dict_len, 65 536) bytes are a virtual prefix in front of every block's output, the target counts from its end -- when the
 *     settings "decompress_partial" and "decompress_shared_dict" are both 1 and "decompress_variant" is not 1; the blocks it hands back
 *     (what the partial form hands back, and a block whose positions would pass 4 GiB - 64 KiB) are decoded again in the reference's
 *     order, sixteen lanes per block, with the dictionary, up to their target (lz4_decompress.hip: the definition above, literally).
 *     Otherwise every block goes through that kernel.  "decompress_second_pass" 0 leaves handed-back blocks marked 0x7F000001.
 *     Measured on an MI355X (tools/partial_dict_bench.py, one session, profiles/r15_partial_dict.txt; blocks compressed against one 32 KiB
 *     dictionary, device-resident, ms per call for 65 536 log records of 4 KiB / 16 384 JSON tiles of 64 KiB): the full
 *     lz4flex_decompress_batch_shared_dict 0.56 / 1.93; this entry at target 64: 0.319 / 0.234, at 512: 0.335 / 0.237 (the set entry, K = 4:
 *     0.335 / 0.233), at 4 096: 0.585 / 0.315, at 65 536: - / 1.942.  "decompress_partial" 0 at the same targets: 0.037 / 0.019, 0.231 /
 *     0.112, 1.80 / 0.712, - / 8.48 -- as for the plain partial entry, the reference's order wins where the target is a few hundred bytes.
 *     A full-size target is level with the full entry on the tiles and 4.5 % slower on the 4 KiB records (the block's last sequence is
 *     cut off its chunk and executed alone): a caller that wants whole blocks calls the full entry.
 * Returns 0 or -code for call-level failures (-LZ4FLEX_E_INVALID_ARG: a missing array -- target counts as one --, dict == NULL with
 * dict_len != 0, a mem_kind other than HOST / DEVICE (| BIG_BLOCKS); the arguments are checked before a context is looked at); n == 0
 * returns 0; -LZ4FLEX_E_NO_DEVICE without a device. */
int lz4flex_decompress_batch_partial_shared_dict(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                                                 uint32_t n, void *out_base, const uint64_t *out_off, const uint32_t *target,
                                                 uint32_t *out_len, int32_t *status, const void *dict, uint32_t dict_len,
                                                 int mem_kind, void *hip_stream);

/* ---- dictionary sets: K prepared dictionaries, one id per block ----------------------------------------------------------------
 * The *_shared_dict entries prepare their one dictionary again on every call (the digest kernel, one wavefront; a MEM_HOST call
 * stages the dictionary again), and a batch whose records belong to a handful of dictionaries -- one per table or per column -- has
 * only the *_ex entries: per-block indexing on the way in, sixteen serial lanes per block on the way back.  A dictionary set is the
 * prepared-dictionary object for both: K dictionaries copied to the device ONCE and digested ONCE, owned by a handle, addressed per
 * block by an id.
 *   lz4flex_dict_set_create: dictionary d is dict_base[dict_off[d] .. + dict_len[d]); mem_kind LZ4FLEX_MEM_HOST or LZ4FLEX_MEM_DEVICE
 *     says where the bytes AND the two arrays lie.  1 <= k <= 1 024 (this library's cap).  dict_len[d] == 0 is legal: id d means "no
 *     dictionary".  The set copies each dictionary's last min(len, 65 536) bytes -- an offset is at most 65 535, so no decoder and no
 *     encoder reads further back -- into device memory it owns, and records the untruncated length (compress_mode exact picks its
 *     table kind from it, src/block/compress.rs:559).  It builds a digest per dictionary (the one lz4flex_compress_batch_shared_dict
 *     builds per call; 41 KiB each) in ONE launch, a workgroup per dictionary.  The digests live in the set, not in a context's
 *     workspace: a shared-dictionary call on the same context does not disturb them.  The call blocks until the set is ready; the
 *     caller may free or overwrite its buffers afterwards.  The set belongs to the context's DEVICE, not to the context: any context
 *     of that device may use it, also several at a time (nothing in it is written after create but a test counter).
 *     -LZ4FLEX_E_INVALID_ARG: out, dict_off or dict_len NULL, k == 0, k > 1 024, a mem_kind other than HOST / DEVICE (checked before a
 *     context is looked at); dict_base NULL with a non-empty dictionary.  -LZ4FLEX_E_NO_DEVICE without a device.
 *   lz4flex_dict_set_free: the caller orders it behind the work that uses the set (a MEM_DEVICE call is asynchronous: synchronise its
 *     stream first).  NULL is harmless.
 *   dict_id (n ids, in the BATCH's memory kind): block i's dictionary is number dict_id[i] of the set.  0xFFFFFFFF: block i has no
 *     dictionary.  Any other id >= k: the block gets status LZ4FLEX_E_INVALID_ARG and out_len 0, nothing of it is written, the rest of
 *     the batch is unaffected.
 *   The calls: everything not said here is as for the *_shared_dict entries.  The arguments are checked before a context is looked
 *     at: -LZ4FLEX_E_INVALID_ARG for a missing array (dict_id is one), set == NULL with n != 0, a mem_kind other than HOST / DEVICE
 *     (| BIG_BLOCKS; LZ4FLEX_MEM_CHAINED is refused); n == 0 returns 0.  A set of another device than the context's: -LZ4FLEX_E_INVALID_ARG.
 *     MEM_DEVICE calls are asynchronous on hip_stream and allocate nothing; MEM_HOST calls stage the batch and the ids, NOT the
 *     dictionaries.
 *   The contract is equality with entries that exist.  Compress: block i gets, byte for byte, what lz4flex_compress_batch_ex gives it
 *     with dictionary dict_id[i] as its per-block dictionary, in both compress modes and under every "compress_sliding_window"; a
 *     block without a dictionary gets what lz4flex_compress_batch gives it in a batch of the same size.  Decompress: block i gets what
 *     lz4flex_decompress_batch_ex gives it with that dictionary and no out_pos -- bytes, out_len, every DecompressError in the
 *     reference's check order, the OutputTooSmall detail counted from out_off.  Nothing is written behind out_len, in front of
 *     out_off, or into the set.
 *   The kernels.  compress_mode fast: a third instance of the throughput encoder's body (lz4_compress_wave.hip, the _set_ kernels)
 *     reads the item's record through its id; an item with a dictionary takes the path it takes in the _shared_ kernels -- the tail
 *     staged from that dictionary's digest, the first window's table from it when hs > 0 and block length >= hs + 11 - h -- every
 *     other item the per-block path; a workgroup keeps the staged tail only from an item to the next of the SAME dictionary.
 *     "compress_shared_dict" 0: no item starts from a digest.  compress_mode exact: the one-block chains of lz4flex_compress_batch_ex,
 *     their records filled from the set's table on the device.  Decompress: the sequence decoder's dictionary form with the
 *     dictionary looked up per block (a block without one decodes in the same launch); the blocks it hands back are decoded in the
 *     reference's order with their own dictionary; "decompress_shared_dict" 0 / "decompress_variant" 1: that order for every block.
 *   Not timed yet: tools/dict_set_bench.py times K = 1 against the *_shared_dict entries (large batches; 256 and 1 024 records per call:
 *     what the prepared digest saves per call), and K = 4 against the *_ex entries with per-block arrays
 *     (profiles/r12_dict_set.txt holds the register figures and awaits the table). */
typedef struct lz4flex_dict_set lz4flex_dict_set;
int lz4flex_dict_set_create(lz4flex_ctx *ctx, const void *dict_base, const uint64_t *dict_off, const uint32_t *dict_len,
                            uint32_t k, int mem_kind, lz4flex_dict_set **out);
void lz4flex_dict_set_free(lz4flex_dict_set *s);
uint32_t lz4flex_dict_set_count(const lz4flex_dict_set *s);
int lz4flex_compress_batch_dict_set(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                                    uint32_t n, const uint32_t *dict_id, void *out_base, const uint64_t *out_off,
                                    const uint32_t *out_cap, uint32_t *out_len, int32_t *status,
                                    const lz4flex_dict_set *set, int mem_kind, void *hip_stream);
int lz4flex_decompress_batch_dict_set(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                                      uint32_t n, const uint32_t *dict_id, void *out_base, const uint64_t *out_off,
                                      const uint32_t *out_cap, uint32_t *out_len, int32_t *status, uint64_t *detail /* nullable */,
                                      const lz4flex_dict_set *set, int mem_kind, void *hip_stream);
/* Partial decode against a set: lz4flex_decompress_batch_partial_shared_dict (its contract, settings and kernels) with block i's
 * dictionary looked up by dict_id[i], the calls as for the two entries above: the arguments are checked before a context is looked at
 * (-LZ4FLEX_E_INVALID_ARG for a missing array -- dict_id and target count --, set == NULL with n != 0, a mem_kind other than HOST / DEVICE
 * (| BIG_BLOCKS)); n == 0 returns 0; a set of another device: -LZ4FLEX_E_INVALID_ARG; -LZ4FLEX_E_NO_DEVICE without a device.  MEM_HOST
 * calls stage the batch (the output staging sized from target[]) and the ids, not the dictionaries.
 *   dict_id[i] == 0xFFFFFFFF, or an id whose dictionary is empty: block i gets what lz4flex_decompress_batch_partial gives it.  A set of K =
 *   1 and every id 0: the results of lz4flex_decompress_batch_partial_shared_dict with that dictionary.  Any other id >= k: status
 *   LZ4FLEX_E_INVALID_ARG, out_len 0, nothing written, the rest of the batch unaffected.  Nothing is written at or behind out_off[i] +
 *   target[i], in front of out_off[i], or into the set. */
int lz4flex_decompress_batch_partial_dict_set(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint32_t *in_len,
                                              uint32_t n, const uint32_t *dict_id, void *out_base, const uint64_t *out_off,
                                              const uint32_t *target, uint32_t *out_len, int32_t *status,
                                              const lz4flex_dict_set *set, int mem_kind, void *hip_stream);

/* Train a dictionary from a batch of samples (lz4_dict_train.hip): sample i is in_base[in_off[i] .. + in_len[i]); the dictionary -- at
 * most dict_cap <= 65 536 bytes, left-aligned in dict_out, *dict_len of them -- is a concatenation of segments of at most `segment`
 * bytes (64 ... 2 048; 0 = 512) cut from the samples.  What it is for: lz4flex_compress_batch_shared_dict / lz4flex_dict_set_create and
 * their decoders, for many small records that have no "earlier part of the file" to use.  The bytes are a function of the samples,
 * dict_cap and segment ALONE (never of the device, the memory kind or the stream): tests/sim/dict_train_model.c is the definition, the
 * kernels equal it byte for byte.  The rule, fastCover's restated so that every step is an integer computation with a fixed result:
 *   a candidate is a position p of a sample with 8 bytes left; candidates are numbered through the batch; total = their number;
 *   hash(p) = (LE64(sample[p .. p + 8)) * 0x9E3779B185EBCA87) >> 44; freq[h] counts the candidates of the whole batch with hash h;
 *   first(p) = 0 if one of the segment - 1 candidates in front of p in its sample has p's hash, else 1;
 *   w(p) = first(p) ? min(freq[hash(p)], 2^20 - 1) : 0; the score of a start s is the sum of w over [s, min(s + segment - 7, candidates
 *   of the sample));  nseg = ceil(dict_cap / segment), E = max(1, min(nseg, total / (4 segment))), R = ceil(total / E);
 *   step t = 0 .. 2 nseg - 1 (until no capacity is left or E steps in a row chose nothing) takes the start with the largest score among
 *   the global numbers [r R, (r + 1) R), r = t mod E, the lowest number among equals, nothing at score 0: the segment is sample[s .. s +
 *   min(segment, in_len - s)), clipped to the capacity left, and the counters of its candidates are set to 0;
 *   the dictionary holds the segments in REVERSE order of choice -- the encoders look at a dictionary's tail, the best material is there.
 * *status: 0, or LZ4FLEX_E_UNSUPPORTED (and *dict_len 0) for 2^32 candidates or more.  Samples may overlap and come in any order; they
 * are only read.  Nothing is written outside dict_out[0 .. *dict_len), dict_len, status and work.
 * mem_kind: LZ4FLEX_MEM_DEVICE -- every pointer is device memory, `work` holds lz4flex_dict_train_work_size(n) bytes (8-byte aligned; 4
 *   MiB of counters and a few words per sample), the call is asynchronous on hip_stream, allocates nothing, copies nothing to the host
 *   and never synchronises: 2 nseg + a few launches whose shape depends on n, dict_cap and segment alone -- or LZ4FLEX_MEM_HOST -- staged
 *   through the context and synchronous; `work` is ignored.  LZ4FLEX_MEM_BIG_BLOCKS may be ORed in (samples of any u32 length are taken
 *   either way); LZ4FLEX_MEM_CHAINED is refused.
 * The arguments are checked before a context or a device is looked at: -LZ4FLEX_E_INVALID_ARG for a segment that is not 0 and outside
 *   64 ... 2 048, dict_cap > 65 536, dict_len or status NULL, dict_out NULL with dict_cap != 0, in_off or in_len NULL with n != 0, a
 *   mem_kind other than HOST / DEVICE (| BIG_BLOCKS), work NULL in a DEVICE call.  n == 0 or dict_cap == 0: returns 0 with *dict_len = 0,
 *   *status = 0 (HOST: without a device; DEVICE: written by a kernel).  -LZ4FLEX_E_NO_DEVICE without a device: there is no CPU path. */
size_t lz4flex_dict_train_work_size(uint32_t n);
int lz4flex_dict_train(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint32_t *in_len, uint32_t n,
                       void *dict_out, uint32_t dict_cap, uint32_t segment /* 0 = 512 */, uint32_t *dict_len /* 1, written */,
                       int32_t *status /* 1, written */, void *work, int mem_kind, void *hip_stream);

/* ---- typed batches: byte- and bit-shuffle filters around the codec (lz4_filter.hip) ---------------------------------------------
 * Numeric data -- bf16 / fp32 weights, int64 ids and timestamps -- compresses far better once the bytes (or bits) of equal significance
 * lie together: LZ4 behind a filter, as HDF5's shuffle / bitshuffle, Blosc and the data_type option of batched GPU LZ4 do it.  The
 * filters are pure byte permutations of a block, defined exactly:
 *
 * A block is `L` bytes. `E` is the element size, one of {1, 2, 4, 8}: fp8/int8, bf16/fp16, fp32/int32, fp64/int64. Both filters map `L`
 * bytes to `L` bytes.
 *
 * - SHUFFLE (1).
 *   - `m = L / E`, rounded down.
 *   - For element `e < m` and byte `j < E`: `out[j*m + e] = in[e*E + j]`.
 *   - The last `L - m*E` bytes are copied unchanged to the same positions.
 *   - `E = 1` is a copy.
 * - BITSHUFFLE (2).
 *   - `m8 = (L / E) / 8 * 8`.
 *   - Plane `p = 8*j + k` holds bit `k` (LSB = 0) of byte `j` of every element, for `j < E` and `k < 8`.
 *   - Plane `p` occupies `out[p*m8/8 .. (p+1)*m8/8)`.
 *   - Bit `b` (LSB = 0) of byte `q` of plane `p` is bit `k` of `in[(8q + b)*E + j]`.
 *   - The last `L - m8*E` bytes are copied unchanged to the same positions.
 *   - In numpy: `packbits(unpackbits(x[:m8*E].reshape(m8, E), axis=1, bitorder='little').T, axis=1, bitorder='little')`.
 *   - This is the arrangement the HDF5 bitshuffle filter gives one whole block, but no file compatibility is claimed. The definition
 *     above is the contract.
 * - The whole block is one transposition, with no sub-blocking. The inverse is the inverse permutation for the same `L` and `E`.
 *   `FILTER_NONE (0)` is a copy.
 * - DELTA (flag 0x10, ORed into one of the three above: the valid values of `filter` are 0, 1, 2, 0x10, 0x11 and 0x12). A difference
 *   stage in front of the base filter, as Parquet's delta encoding and Blosc's delta filter have one: in a monotone column -- timestamps,
 *   sorted ids -- neighbours differ by little, and the differences' high planes are runs where the values' low planes are noise. It does
 *   not help floating-point weights, so it is never a default.
 *   - Forward. `m = L / E`. Element `x[e]` is the little-endian unsigned integer of `E` bytes at `in[e*E]`.
 *     `d[e] = x[e]` where `e % LZ4FLEX_DELTA_RESTART == 0`, otherwise `d[e] = (x[e] - x[e-1]) mod 2^(8E)`. The last `L - m*E` bytes stay
 *     where they are. The forward typed filter is the base filter (same `L` and `E`) applied to the block of `d`.
 *   - Inverse. The base filter's inverse, then `x[e] = (d[r] + ... + d[e]) mod 2^(8E)` with `r = e - e % LZ4FLEX_DELTA_RESTART`.
 *   - The restart every 1 024 elements keeps a tile's work inside one wavefront (no scan over the block, no workspace, one launch) and
 *     costs nothing in ratio.
 *   - `E = 1` is a bytewise delta; `DELTA | SHUFFLE` with `E = 1` is the delta alone. With BITSHUFFLE, the up to 7 elements behind `m8`
 *     are differenced like all the others; only their placement is "unchanged".
 *   - `E = 2`, `L = 7`: `01 00 03 00 02 00 AA` becomes `01 00 02 00 FF FF AA` (DELTA alone).
 *   - `E = 1`, `L = 1026`, every byte 5: the result is 5, then 1 023 zeros, then 5, then 0.
 *   - Everything below holds with the flag set; `filter != LZ4FLEX_FILTER_NONE` includes 0x10: a DEVICE call with the flag needs tmp.
 *
 * lz4flex_filter_batch: block i's in_len[i] bytes at in_base + in_off[i] are transformed (inverse != 0: by the inverse permutation) into
 *   out_base + out_off[i]; offsets of any alignment; overlapping input and output regions are the caller's error.
 * lz4flex_compress_batch_typed: the forward filter of every block goes into tmp_base + tmp_off[i] (a slot holds at least in_len[i]
 *   bytes; typically a second buffer of the input's size with tmp_off = in_off), then the ordinary batch path runs with the slots as
 *   input.  out, out_len and status are byte for byte what lz4flex_compress_batch (flags NULL) gives for the filtered bytes in a batch of
 *   the same n, under the same settings, in every compress mode.
 * lz4flex_decompress_batch_typed: lz4flex_decompress_batch runs into the tmp slots with capacity out_cap[i] (a slot holds at least
 *   out_cap[i] bytes), then the inverse filter runs over L = out_len[i] of every block with status 0 -- read from the device arrays on the
 *   same stream -- into out_base + out_off[i].  out_len, status and detail are exactly lz4flex_decompress_batch's; a block with status != 0
 *   writes nothing to out_base; nothing is written behind out_off[i] + out_len[i] or in front of out_off[i].
 * All three: filter == LZ4FLEX_FILTER_NONE behaves as the plain entry (lz4flex_filter_batch: as a copy) and does not touch tmp.  Nothing
 *   outside [off, off + L) of a block is read or written, on either side.
 * mem_kind: LZ4FLEX_MEM_DEVICE -- every pointer is device memory, asynchronous on hip_stream, nothing is allocated (one launch per
 *   filter pass) -- or LZ4FLEX_MEM_HOST -- staged through the context and synchronous; tmp_base and tmp_off are ignored, the staging
 *   arena holds the slots.  LZ4FLEX_MEM_BIG_BLOCKS may be ORed in (the codec reads it as in the plain entries; lz4flex_filter_batch takes
 *   blocks of any u32 length either way); LZ4FLEX_MEM_CHAINED is refused.
 * The arguments are checked before a context or a device is looked at: -LZ4FLEX_E_INVALID_ARG for an unknown filter, elem_size outside
 *   {1, 2, 4, 8}, a mem_kind other than HOST / DEVICE (| BIG_BLOCKS) and, with n != 0, a missing array, or a missing tmp_base / tmp_off in a
 *   DEVICE call with filter != NONE.  n == 0 returns 0.  -LZ4FLEX_E_NO_DEVICE without a device: there is no CPU path.
 * Setting "filter_bytewise" (A/B measurements, tests): 1 = the kernels take every block by their narrow path (byte accesses), 0 (default)
 *   = 16-byte accesses wherever every 16-byte store of a block can be aligned.  Not in scope: dictionaries, frames (the LZ4 frame header has
 *   no field for a filter), the CLI. */
#define LZ4FLEX_FILTER_NONE 0
#define LZ4FLEX_FILTER_SHUFFLE 1
#define LZ4FLEX_FILTER_BITSHUFFLE 2
#define LZ4FLEX_FILTER_DELTA 0x10
#define LZ4FLEX_DELTA_RESTART 1024
int lz4flex_filter_batch(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint32_t *in_len, uint32_t n,
                         void *out_base, const uint64_t *out_off, int filter, uint32_t elem_size, int inverse, int mem_kind,
                         void *hip_stream);
int lz4flex_compress_batch_typed(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint32_t *in_len, uint32_t n,
                                 void *out_base, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len, int32_t *status,
                                 int filter, uint32_t elem_size, void *tmp_base, const uint64_t *tmp_off, int mem_kind,
                                 void *hip_stream);
int lz4flex_decompress_batch_typed(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint32_t *in_len, uint32_t n,
                                   void *out_base, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len, int32_t *status,
                                   uint64_t *detail /* nullable: 2 per block */, int filter, uint32_t elem_size, void *tmp_base,
                                   const uint64_t *tmp_off, int mem_kind, void *hip_stream);

/* ---- fit batches: compress into a fixed capacity (lz4_fit.hip) -- liblz4's LZ4_compress_destSize as a batch -----------------------
 * "How much of my input fits in this slot?"  lz4flex_fit_batch cuts a FINISHED block to a capacity; lz4flex_compress_batch_fit runs the
 * batch encoder in front of it.  The compress-side mirror of lz4flex_decompress_batch_partial.
 *
 * THE RULE (tests/fit_model.py is the same rule as a program).  Given a valid block `B` with sequences `j = 0 .. S-1` (literals `l_j`,
 * match `m_j`, offset `d_j`; the last one has no match), the `n` source bytes `B` decodes to, and a capacity `cap`.  Write `c_j` for the
 * compressed offset of sequence j's token and `p_j` for its decoded offset, and
 *     `ext(x) = 0 if x < 15 else 1 + (x-15)/255`          (integer division: the length bytes behind a token's nibble)
 *     `tail(L) = 1 + ext(L) + L`                           (a final run of L literals, compressed)
 *     `Lfit(r, avail)` = the largest `L` in `[0, avail]` with `tail(L) <= r`.
 *   1. `B` fits: if `len(B) <= cap`, the output is `B` byte for byte, `in_used = n`, and nothing is walked.
 *   2. `B` does not fit: the best candidate over all `k` with `c_k < cap`.
 *      Plain(k): sequences `0 .. k-1` unchanged, then a final run of `L = Lfit(cap - c_k, n - p_k)` literals.  Legal iff `L >= Lmin`,
 *        `Lmin = 0` for `k = 0`, else `max(5, 12 - m_{k-1})` (the format's end rules: the last 5 bytes are literals, the last match
 *        starts at least 12 bytes before the end).  `used = p_k + L`, `size = c_k + tail(L)`.
 *      Clipped(k), only when `m_k >= 5`: sequences `0 .. k-1`, then sequence `k` with its literals and its match cut to `m'`, then a
 *        final run `L`.  With `h = 1 + ext(l_k) + l_k + 2` and `b = cap - c_k - h - 1` it needs `b >= 5`;
 *        `m' = min(m_k - 1, 18 + 255*(b - 5))`, and `max(5, 12 - m') <= b` is required;
 *        `L = Lfit(cap - c_k - h - ext(m'-4), n - p_k - l_k - m')`, legal iff `L >= max(5, 12 - m')`.
 *        `used = p_k + l_k + m' + L`, `size = c_k + h + ext(m'-4) + tail(L)`.
 *      A candidate whose sequences alone decode to more than `n` bytes (`p_k > n`, `p_k + l_k + m' > n`: a wrong src_len) is not legal.
 *      Choice: the largest `used`; ties go to the smallest size, then the smallest `k`, then Plain before Clipped.  The maximum is over
 *        EVERY such k, not the last one alone (a sequence with `l >= 15`, `m = 4` costs as many compressed bytes as it decodes).
 *      The final literals are read from the source at the decoded position: `src[used - L, used)`.
 *   3. No candidate -- only at `cap == 0`: status LZ4FLEX_E_OUTPUT_TOO_SMALL, out_len 0, in_used 0, nothing is written.
 *   Errors: every sequence whose token lies in front of cap (`c_k < cap`) is parsed in the reference's check order
 *   (decompress.rs:249-443: all of its length bytes, its offset, the token that must follow a match), and the first error met is the
 *   block's status -- the DecompressError code, out_len 0, in_used 0, nothing written.  Nothing of a sequence at or behind cap is looked
 *   at: an error there is not seen (the partial decoder's contract), and neither is any error of a block that fits.
 *
 * lz4flex_fit_batch: block i = blk_len[i] bytes at blk_base + blk_off[i], its source the src_len[i] bytes at src_base + src_off[i], cut to
 *   out_cap[i] bytes at out_base + out_off[i]; out_len[i] = the bytes written, in_used[i] = the source bytes they decode to, status[i] = 0
 *   or a code as above.  src_len[i] is the caller's promise of what block i decodes to; it is not checked -- with a wrong promise the
 *   output is still a structurally valid block inside out_cap[i], its content unspecified.  Nothing outside [out_off[i], out_off[i] +
 *   out_len[i]) is written, nothing of a block at or behind blk_len[i] and nothing of a source at or behind src_len[i] is read.  The
 *   primitive does not know which encoder wrote the block: every "compress_mode" alike.  It takes SELF-CONTAINED blocks only: there is no
 *   history input, so a block compressed against a dictionary or against a stream's history, whose matches reach in front of its own
 *   output, is refused with LZ4FLEX_E_OFFSET_OUT_OF_BOUNDS where such a match lies in front of the cut (it is copied where it fits whole).
 * lz4flex_compress_batch_fit: lz4flex_compress_batch (no flags, the context's settings) into `scratch`, slots of
 *   lz4flex_get_maximum_output_size(in_len[i]) bytes back to back whose offsets are scanned on the device -- scratch_cap >=
 *   lz4flex_compress_packed_scratch_bound(sum of in_len, n, 0) always suffices; a block whose slot ends behind scratch_cap gets
 *   LZ4FLEX_E_OUTPUT_TOO_SMALL (the packed entry's rule) -- then the fit pass from the slots.  Block i's result is exactly
 *   fit(lz4flex_compress_batch's bytes for the same batch under the same settings, its input, out_cap[i]), in "compress_mode" 0, 1 and 2
 *   alike; out_cap[i] >= lz4flex_get_maximum_output_size(in_len[i]) gives lz4flex_compress_batch's bytes and in_used[i] = in_len[i].  A
 *   block the encoder fails keeps that status (out_len 0, in_used 0).  work: lz4flex_compress_fit_work_size(n) bytes, 8-byte aligned.
 *   Known cost: the encoder encodes all in_len[i] bytes whatever out_cap[i] is.
 * mem_kind: LZ4FLEX_MEM_DEVICE -- every pointer is device memory, asynchronous on hip_stream, nothing is allocated; lz4flex_fit_batch is one
 *   launch plus the launch for the blocks it hands to its reference-order pass -- or LZ4FLEX_MEM_HOST -- staged through the context and
 *   synchronous; scratch and work are ignored.  LZ4FLEX_MEM_BIG_BLOCKS may be ORed in (lz4flex_fit_batch: changes nothing; the encoder reads
 *   it as in the plain entry); LZ4FLEX_MEM_CHAINED is refused.
 * The arguments are checked before a context or a device is looked at: -LZ4FLEX_E_INVALID_ARG for a mem_kind other than HOST / DEVICE
 *   (| BIG_BLOCKS) and, with n != 0, a missing array (DEVICE: a missing scratch or work).  n == 0 returns 0.  -LZ4FLEX_E_NO_DEVICE without a
 *   device: there is no CPU path.
 * Setting "fit_serial" (tests, A/B): 1 = every block is cut by the reference-order pass, a lane per block; 0 (default) = a wavefront per
 *   block, that pass for the blocks it gives up (every error among them).  Same results.
 * Not in scope: flags, dictionaries, history (neither entry takes them; lz4flex_fit_batch with a per-block history length is the
 *   follow-up that would let a caller compose them), frames. */
int lz4flex_fit_batch(lz4flex_ctx *ctx, const void *blk_base, const uint64_t *blk_off, const uint32_t *blk_len, const void *src_base,
                      const uint64_t *src_off, const uint32_t *src_len, uint32_t n, void *out_base, const uint64_t *out_off,
                      const uint32_t *out_cap, uint32_t *out_len, uint32_t *in_used, int32_t *status, int mem_kind, void *hip_stream);
size_t lz4flex_compress_fit_work_size(uint32_t n);
int lz4flex_compress_batch_fit(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint32_t *in_len, uint32_t n,
                               void *scratch, uint64_t scratch_cap, void *out_base, const uint64_t *out_off, const uint32_t *out_cap,
                               uint32_t *out_len, uint32_t *in_used, int32_t *status, void *work, int mem_kind, void *hip_stream);

/* ---- paged streams: every stream cut into pages of page_size bytes, the loop on the device (lz4_paged.hip) ---------------------------
 * "Cut each of my n streams into pages of P bytes."  Every page is a self-contained LZ4 block that holds as much of its stream as fits,
 * page j + 1 starts where page j stopped: the LZ4_compress_destSize loop of fixed-output compression, with no host round trip between
 * pages.  The read side exists: a page is an ordinary block, lz4flex_decompress_batch over the page table puts a stream back together,
 * lz4flex_decompress_batch_partial reads into a page, and lz4flex_paged_read_ranges (below) reads byte ranges of the streams in one call.
 *
 * THE RULE (tests/paged_model.py is the same rule as a program).  P = page_size; stream i is the in_len[i] bytes at in_base + in_off[i]
 * and owns the table entries `[page_off[i], page_off[i+1])`, its capacity `C_i = page_off[i+1] - page_off[i]` pages.  Its state is
 * `pos = 0`, `W = window_min`, `k = 0`.  A stream with `in_len == 0` is finished at once with 0 pages and status 0; a stream with
 * `in_len != 0` and `C_i == 0` ends at once with LZ4FLEX_E_OUTPUT_TOO_SMALL.  One ROUND, for every stream that is still live:
 *   Offer `w = min(W, in_len - pos)`.  `(block, out_len, used, st)` is the result of lz4flex_compress_batch_fit for the window
 *     `src[pos, pos + w)` at capacity P, computed in ONE batch that holds all n streams' windows of this round -- a stream that is not
 *     live has an empty window at capacity 0 whose result is ignored -- so n is the same in every round, and the bytes of
 *     "compress_mode" 0, which depend on n through "compress_subwindows", are those of that one batch.
 *   `st != 0`: the stream ends with that status; its pages so far stay valid.
 *   Retry: `used == w`, `pos + w < in_len` and `W < window_max`.  Nothing is committed, `W = min(2 * W, window_max)`: the window fit
 *     whole, so a larger one might fill the page better.
 *   Commit otherwise: entry `e = page_off[i] + k`, `page_len[e] = out_len`, `page_src[e] = pos`, the block is the first out_len bytes of
 *     page e at `out_base + e * P`; `pos += used`, `k += 1`.  If `pos == in_len` the stream is finished with status 0; else if
 *     `k == C_i` it is out of pages and ends with LZ4FLEX_E_OUTPUT_TOO_SMALL.
 *   A stream that is still live after max_rounds rounds ends with LZ4FLEX_E_OUTPUT_TOO_SMALL; `n_pages[i] < C_i` tells the two causes apart.
 * Results: per stream `n_pages[i] = k`, `in_done[i] = pos`, status[i]; per committed entry page_len, page_src and the page's bytes.
 * Invariants: page e decodes to `src[page_src[e], page_src[e+1])` (the last page of a stream: up to in_done[i]); pages are independent of
 *   each other, any LZ4 block decoder reads them; every committed page of a stream that has more to come consumed at least
 *   `Lfit(P, infinity)` bytes (Lfit: the fit rule's function above; Plain(0) is always a candidate), so `used >= 1` and the loop ends; W
 *   only grows, so a stream retries at most as often as window_min doubles up to window_max.  Hence the two bounds, pure host functions
 *   that need no device: lz4flex_paged_pages_bound(in_len, page_size) = `ceil(in_len / Lfit(page_size, infinity))` -- a capacity that
 *   always suffices -- and lz4flex_paged_rounds_bound(max_in_len, page_size, window_min, window_max) = that bound plus the number of
 *   doublings from window_min to window_max (0 selects the defaults, as below) -- a max_rounds that always suffices.  Both return 0 for
 *   arguments the entry refuses.
 * Why windows: a round encodes every byte it is offered, so the work follows what a page holds (a few window lengths), not what is left
 *   of the stream.  Why they double: a window that fits a page whole says nothing about how much more would have fit; data that
 *   compresses better than window_max / P leaves its pages underfilled (a run of zeros: window_max bytes per page, whatever P is).
 * Arguments: `64 <= page_size <= 4 MiB`, `page_size <= window_min <= window_max <= 2^31`; 0 selects the defaults `window_min = 4 *
 *   page_size`, `window_max = max(window_min, 65536)`.  Anything else is -LZ4FLEX_E_INVALID_ARG, and so are a mem_kind other than HOST /
 *   DEVICE (| BIG_BLOCKS; LZ4FLEX_MEM_CHAINED is refused) and, with n != 0, a missing array (DEVICE: a missing scratch or work; HOST: a
 *   page_off that counts down).  The arguments are checked before a context or a device is looked at; n == 0 returns 0;
 *   -LZ4FLEX_E_NO_DEVICE without a device.  page_off has n + 1 values, counted in ENTRIES, not bytes.
 * What may be written: the page file `[out_base, out_base + page_off[n] * P)` -- the bytes of a page behind its page_len are unspecified,
 *   and so are the pages at or behind n_pages[i] --, the table entries of committed pages, the three per-stream results.  Nothing else:
 *   table entries at or behind n_pages[i] stay untouched.
 * mem_kind: LZ4FLEX_MEM_DEVICE -- every pointer is device memory, asynchronous on hip_stream, nothing is allocated and nothing is
 *   synchronised; exactly max_rounds rounds are enqueued, each one the launches of lz4flex_compress_batch_fit plus one step kernel, a
 *   lane per stream (a round in which no stream is live still costs its launches: size max_rounds by what the data can need, not by the
 *   bound, when that is known).  scratch: `scratch_cap >= lz4flex_compress_packed_scratch_bound(sum of min(in_len[i], window_max), n, 0)`
 *   always suffices; a window whose slot ends behind scratch_cap fails its stream with the encoder's LZ4FLEX_E_OUTPUT_TOO_SMALL, as in the
 *   fit entry.  work: lz4flex_compress_paged_work_size(n) bytes, 8-byte aligned.  in_done and n_pages hold the loop's state between rounds.
 *   LZ4FLEX_MEM_HOST -- staged through the context and synchronous; the number of rounds is min(max_rounds, the rounds bound of the
 *   longest stream), computed from the host-visible lengths; scratch and work are ignored.  LZ4FLEX_MEM_BIG_BLOCKS is passed through
 *   to the encoder in every round (HOST: also set when a window can be longer than 64 KiB).
 * The context's settings apply unchanged: "compress_mode" 0 / 1 / 2, "compress_depth", "compress_parse", "fit_serial".
 * Not in scope: dictionaries, history or linked pages (they need the fit pass's history form, the follow-up named above), filters,
 *   frames, an early stop inside the encoders. */
int lz4flex_compress_paged(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint32_t *in_len, uint32_t n,
                           uint32_t page_size, uint32_t window_min, uint32_t window_max, uint32_t max_rounds, void *out_base,
                           const uint64_t *page_off /* n + 1, entries */, uint32_t *page_len, uint32_t *page_src, uint32_t *n_pages,
                           uint32_t *in_done, int32_t *status, void *scratch, uint64_t scratch_cap, void *work, int mem_kind,
                           void *hip_stream);
size_t lz4flex_compress_paged_work_size(uint32_t n);
uint64_t lz4flex_paged_pages_bound(uint32_t in_len, uint32_t page_size);
uint32_t lz4flex_paged_rounds_bound(uint32_t max_in_len, uint32_t page_size, uint32_t window_min, uint32_t window_max);

/* ---- paged streams, the read side: m byte ranges in one call, planned on the device (lz4_paged_read.hip, paged_range.h) ---------------
 * "Give me bytes [a, a + len) of stream i", m times, from the page file and the tables lz4flex_compress_paged wrote -- where it wrote
 * them: in MEM_DEVICE the plan (which pages, which of them from the middle), the decode batches, the gather and the verdicts all run on
 * the device; nothing is read back, nothing is allocated, nothing is synchronised.  The first eight arguments are what
 * lz4flex_compress_paged produced: entry e of the table is the page at `pages + e * page_size`, e is absolute and page_off[0] need not
 * be 0.  What lz4flex_frame_read_ranges is for indexed frames, with the plan on the device because the tables are born there.
 *
 * THE RULE (tests/paged_read_model.py is the same rule as a program; paged_range.h holds its integer part for the host and the kernels).
 * Locating.  For range r: `i = range_stream[r]`, `first = page_off[i]`, `C = page_off[i+1] - first` (0 where page_off counts down),
 *   `k = min(n_pages[i], C)`, `S = in_done[i]`.  `out_len[r] = min(range_len[r], S - range_off[r])`, 0 for `range_off[r] >= S`: a read at
 *   end of file.  Those bytes are stream i's bytes at that position, written at `out_base + out_off[r]`.  Writes are strict: nothing in
 *   front of that address, nothing at or behind `+ out_len[r]`, nothing else of out_base, nothing of the tables or the page file.  The
 *   page that holds stream byte pos is the last `j < k` with `page_src[first + j] <= pos`; page j decodes to `[page_src[first+j],
 *   page_src[first+j+1])`, the last page up to S.  A range touches pages `j0 .. j1`, `nb = j1 - j0 + 1`.
 * Which page decodes where.  Every touched page whose start lies inside the range is decoded straight into the output
 *   (lz4flex_decompress_batch_partial with target = the page's wanted bytes; the last page is clipped at the range's end).  If the range
 *   starts inside page j0 (`s = range_off - page_src[first+j0] > 0`) that page is a HEAD: it is decoded into `scratch` up to its last
 *   wanted byte, `head_bytes = min(range end, page end) - page start`, and `[s, head_bytes)` is copied out.  LZ4 has no other way into a
 *   page than its first byte.  Several ranges that hit one page decode it once each.
 * Capacities, in range order.  `slot_r` = the sum of nb over the ranges in front of r (whatever became of them); `head_off_r` = the sum
 *   of their head_bytes, each rounded up to 64.  Range r is SERVED iff `slot_r + nb_r <= max_items` and, when it has a head,
 *   `head_off_r + head_bytes_r <= scratch_cap` (a range without a head takes no scratch and is never refused for it).  A range that is
 *   not served gets LZ4FLEX_E_OUTPUT_TOO_SMALL and out_len 0, nothing of it is written, the other ranges are unaffected -- the packed and
 *   fit entries' rule.  lz4flex_paged_range_pages_bound(L, P), a pure host function: 0 for L = 0, 1 for L = 1, else
 *   `2 + (L - 2) / Lfit(P, infinity)` -- the pages between a range's first and last page are non-final pages of their stream, and
 *   lz4flex_compress_paged guarantees each of those at least Lfit(P, infinity) bytes; the first and the last page hold at least one byte of
 *   the range each; 0 for a page size the paged entry refuses.  The sum of the bounds over the ranges is a max_items that always suffices
 *   for tables lz4flex_compress_paged wrote; `m * roundup64(window_max)` is a scratch_cap that always suffices -- real needs are about one
 *   page's decoded size per head.
 * status[r], in this order (codes are positive, as in the batch entries):
 *   1. `range_stream[r] >= n`: LZ4FLEX_E_INVALID_ARG.
 *   2. clipped length 0: status 0, out_len 0, nothing planned.
 *   3. not served: LZ4FLEX_E_OUTPUT_TOO_SMALL.
 *   4. a table that contradicts itself for this range: LZ4FLEX_E_INVALID_ARG, nothing written.  That is: `k == 0` with bytes wanted; a
 *      touched page with `page_len > page_size`, one that starts at or behind S, or at or behind the start of the page behind it (page_src
 *      not ascending over the touched pages); a first page that does not hold range_off, another page that does not start inside the
 *      range, a last page that ends in front of the range's end -- every item's output span lies inside `[0, out_len)` or its head slot.
 *   5. the first touched page, in stream order, that does not deliver: the partial decoder's error code if it fails the page;
 *      LZ4FLEX_E_EXPECTED_ANOTHER_BYTE if the page decodes without an error but to fewer bytes than wanted (the page ended before the
 *      table says it does -- deliberately another code than the capacity code of 3).
 *   On any error out_len[r] = 0; under 5 the range's own region may hold anything.
 * Hostile tables (MEM_DEVICE: caller-supplied device memory): whatever page_len / page_src / n_pages / in_done hold, no page is read
 *   outside `pages[e * P, e * P + P)` of an entry e inside the stream's `[first, first + C)`, and nothing is written outside a range's
 *   region or its head slot: condition 4 is checked for every touched page of a served range before an item exists.
 * Call-level returns, checked before a context or a device is looked at: -LZ4FLEX_E_INVALID_ARG for a mem_kind other than HOST / DEVICE
 *   (| BIG_BLOCKS, which is passed to the decoder; LZ4FLEX_MEM_CHAINED is refused) and for a page_size outside 64 .. 4 MiB; then m == 0
 *   returns 0; then -LZ4FLEX_E_INVALID_ARG for a missing array (the five tables, the three range arrays, out_off, out_len, status) and, in
 *   DEVICE mode, a missing work or a missing scratch with scratch_cap != 0.  -LZ4FLEX_E_NO_DEVICE without a device.
 * mem_kind: LZ4FLEX_MEM_DEVICE -- every pointer is device memory, asynchronous on hip_stream; a fixed sequence of launches, all sized by m
 *   and max_items: locate (a lane per range), two offset scans (lz4_packed.hip's), check (a wavefront per range) and emit (a thread per
 *   item slot), lz4flex_decompress_batch_partial over max_items bodies and over m heads, the gather, the verdict (a wavefront per
 *   range).  A slot nobody owns is a one-byte block with target 0 -- the partial decoder reads nothing of it -- so an oversized max_items
 *   costs empty decoder slots and the work arrays, not decode time.  work: lz4flex_paged_read_work_size(m, max_items) bytes, 8-byte
 *   aligned; scratch and work may be overwritten.  "decompress_partial" picks the partial decoder as for lz4flex_decompress_batch_partial.
 *   LZ4FLEX_MEM_HOST -- everything is host memory, staged through the context and synchronous; max_items, scratch, scratch_cap and work
 *   are ignored: the host locates the ranges itself and sizes exactly (no range is refused under 3).  Per range ONE upload of the span of
 *   its touched pages goes up and its bytes come back: a small read does not upload the page file.  The ranges are cut into passes under
 *   the setting "frame_range_pass_bytes" (a pass takes at least one range).
 * Measured on an MI355X (tools/paged_read_bench.py, one session, profiles/r25_paged_read.txt; device-resident, ms per call, host clock
 *   around a synchronised call): 16 384 x 64 KiB JSON tiles in 4 KiB pages, every stream as one range 2.31 (block.decompress_paged_device
 *   on the same tables, its synchronisation included: 2.46); 1 024 / 65 536 random 4 KiB ranges 0.26 / 1.96 (1 272 / 81 164 touched
 *   pages); 65 536 ranges of 64 bytes 1.39.  A small call is bound by its dozen launches, a large one scales with the touched pages.
 * Not in scope: dictionaries, history and filters on pages; de-duplicating ranges that hit one page; a skip-ahead decoder for heads. */
uint32_t lz4flex_paged_range_pages_bound(uint32_t range_len, uint32_t page_size);
size_t lz4flex_paged_read_work_size(uint32_t m, uint32_t max_items);
int lz4flex_paged_read_ranges(lz4flex_ctx *ctx, const void *pages, uint32_t page_size, const uint64_t *page_off /* n + 1, entries */,
                              const uint32_t *page_len, const uint32_t *page_src, const uint32_t *n_pages, const uint32_t *in_done,
                              uint32_t n, const uint32_t *range_stream, const uint32_t *range_off, const uint32_t *range_len, uint32_t m,
                              void *out_base, const uint64_t *out_off, uint32_t *out_len, int32_t *status, uint32_t max_items,
                              void *scratch, uint64_t scratch_cap, void *work, int mem_kind, void *hip_stream);

/* ---- paged streams, append: new bytes for any subset of the streams, the tail page reopened (lz4_paged_append.hip, paged_append.h) -----
 * "Here are more bytes for some of my n paged streams."  One call, planned on the device in MEM_DEVICE: every stream that gets bytes has
 * its last page decoded again, the new bytes put behind it, and the paged rule of lz4flex_compress_paged resumed over the two -- so the
 * old last page is filled up before a new one is begun, the work follows the new bytes and not the stream's length, and the source of
 * what is already paged is not needed.  The tables are those lz4flex_compress_paged wrote, with room behind n_pages[i] (entries up to
 * page_off[i+1]) for the pages to come.
 *
 * THE RULE (tests/paged_append_model.py is the same rule as a program; paged_append.h holds its integer part for the host and the kernels).
 * P = page_size.  On entry stream i has `first = page_off[i]`, `C = page_off[i+1] - first`, `k = n_pages[i]`, `S = in_done[i]` and
 * `A = add_len[i]` new bytes at `add_base + add_off[i]`.  Whatever status[i] held on entry is ignored: a stream that ended
 * LZ4FLEX_E_OUTPUT_TOO_SMALL earlier continues from its in_done.
 *   1. `A == 0`: the stream takes no part, nothing of it is touched; `status[i] = 0`, `stage_off[i] = ~0`, `tail_src[i] = S`.
 *   2. A table that contradicts itself: LZ4FLEX_E_INVALID_ARG, nothing of the stream is written (`stage_off[i] = ~0`, `tail_src[i] = S`).
 *      That is: page_off counting down; `k > C`; `k == 0` with `S != 0`; with `k > 0` a last entry `e = first + k - 1` with
 *      `page_len[e] == 0`, `page_len[e] > P`, `page_src[e] >= S` or `T = S - page_src[e] > window_max` (no page that
 *      lz4flex_compress_paged wrote at that window_max holds more than a window); `S + A > 2^32 - 1`.
 *   3. The tail: `base = page_src[e]`, `T = S - base`; with `k == 0`: `base = 0`, `T = 0`.  `tail_src[i] = base`.
 *   4. Staging: stream i needs `roundup64(T + A)` bytes of `stage`; its slot starts at the sum of those sizes over the streams in front
 *      of it that passed 2.  A stream whose slot ends behind stage_cap is not served: LZ4FLEX_E_OUTPUT_TOO_SMALL, `stage_off[i] = ~0`,
 *      nothing of it is touched, the other streams are unaffected.  A served stream gets `stage_off[i]` = its slot.
 *      lz4flex_paged_append_stage_bound(sum of add_len, n, window_max) = `sum_add_len + n * (window_max + 63)` is a stage_cap that always
 *      suffices; window_max 0 stands for 65536, the default of every page size up to 16 KiB at the default window_min -- pass the resolved
 *      window_max otherwise; 0 for a window_max below 64 or above 2^31.
 *   5. Reopen: the last page is decoded into the slot (lz4flex_decompress_batch_partial at target T) and the new bytes are copied behind
 *      it.  A tail page that fails gives the decoder's code; one that decodes to fewer than T bytes gives LZ4FLEX_E_EXPECTED_ANOTHER_BYTE.
 *      In both cases the stream's tables and pages stay untouched.
 *   6. Resume: the stream runs the rule of lz4flex_compress_paged unchanged, in the same rounds as the others, over the virtual stream
 *      `V = tail ++ add` of T + A bytes: it starts at `W = window_min`, `pos = base` and page index `k - 1` (0 with `k == 0`), so entry
 *      `first + k - 1` is overwritten and the entries behind it are taken up to C.  A stream that is not served, failed or has `A == 0` is
 *      a dead stream in every round (an empty window at capacity 0), so n is the same in every round.  page_src values are stream
 *      positions, `base + (position in V)`.  On return n_pages, in_done and status are the loop's results.  On a nonzero status from the
 *      rounds the tables describe a valid prefix `[0, in_done)`: in_done may be smaller than S, never smaller than base, and the bytes
 *      not yet paged are at `stage + stage_off[i] + (in_done[i] - tail_src[i])`, so nothing is lost.
 * What it equals: for a served stream the entries from `first + k - 1` on, their pages' first page_len bytes, `n_pages - (k - 1)`,
 *   `in_done - base` and status are those of ONE lz4flex_compress_paged call over n streams -- stream i is V_i, or empty for a dead
 *   stream -- with the same n, windows, max_rounds and settings at capacity `C - (k - 1)` (C with `k == 0`); page_src there counts from 0.
 * Invariants: every page but a stream's last still holds at least `Lfit(P, infinity)` bytes after any sequence of appends -- the reopened
 *   page was the last one, and every page committed in front of a new last one is committed by the paged rule with more to come.  Hence
 *   `n_pages <= lz4flex_paged_pages_bound(in_done, P)` however many appends there were, a capacity of the bound for the final length always
 *   suffices, lz4flex_paged_range_pages_bound stays valid, and `lz4flex_paged_rounds_bound(window_max + the longest add_len, ...)` rounds
 *   always suffice.
 * What may be written: the pages and the table entries from the reopened entry up to the new n_pages (page bytes behind page_len and
 *   pages at or behind n_pages are unspecified, as for lz4flex_compress_paged), the three per-stream results, stage_off, tail_src,
 *   stage, scratch, work.  Nothing else: table entries at or behind the new n_pages and in front of the reopened entry stay as they are.
 * Hostile tables (MEM_DEVICE: caller-supplied device memory): whatever they hold, no page is read outside `pages[e * P, e * P + P)` of
 *   an entry inside the stream's `[first, first + C)`, nothing is written outside the stream's entries, pages and stage slot: 2 is
 *   checked before an item exists.
 * Call-level returns, in the order of lz4flex_compress_paged and before a context or a device is looked at: -LZ4FLEX_E_INVALID_ARG for
 *   the page size and the windows (same limits and defaults), then for a mem_kind other than HOST / DEVICE (| BIG_BLOCKS;
 *   LZ4FLEX_MEM_CHAINED is refused); then n == 0 returns 0; then -LZ4FLEX_E_INVALID_ARG for a missing array (add_off, add_len, the five
 *   tables, status, stage_off, tail_src; DEVICE: a missing work, scratch or stage).  -LZ4FLEX_E_NO_DEVICE without a device.
 * mem_kind: LZ4FLEX_MEM_DEVICE -- every pointer is device memory, asynchronous on hip_stream, nothing is allocated and nothing is
 *   synchronised.  The launches are fixed and sized by n and max_rounds: locate, the offset scan (lz4_packed.hip's), emit, the partial
 *   decode over n tail items, the copy batch over n add items, resume, then max_rounds x (lz4flex_compress_batch_fit + the paged step).
 *   A slot nobody owns is a one-byte block with target 0, which the partial decoder answers without reading anything.  scratch:
 *   `lz4flex_compress_packed_scratch_bound(sum of min(T_i + add_len[i], window_max), n, 0)` suffices (T_i = window_max where it is not
 *   known on the host).  work: lz4flex_paged_append_work_size(n) bytes, 8-byte aligned.  LZ4FLEX_MEM_BIG_BLOCKS goes to the decoder and to
 *   the encoder.  LZ4FLEX_MEM_HOST -- staged through the context and synchronous; stage, scratch, work and their capacities are ignored
 *   and no stream is refused under 4.  Only the tables, each appended stream's last page and the new bytes go up; only the entries and
 *   pages from the reopened one on -- as many as T + A bytes can take by the pages bound, whatever room the table keeps behind them --
 *   and the results come down, copied to their places.  Rounds = min(max_rounds, the rounds bound of the
 *   longest T + A).  There is no caller-visible stage: stage_off[i] is ~0 for every stream, tail_src[i] is reported; a caller that needs
 *   the unpaged bytes back after a nonzero status uses the device form.
 * Kernels (lz4_paged_append.hip; a lane per stream each, no LDS, no atomics, no scratch memory): locate 24, emit 26, resume 36 VGPRs.
 * Measured on an MI355X (tools/paged_append_bench.py, one session with the legs alternating, profiles/r26_paged_append.txt; device-resident,
 *   ms per call, host clock around a synchronised call, max_rounds = the rounds bound of what the leg encodes): 16 384 x 64 KiB JSON tiles
 *   in 4 KiB pages appended by 256 B / 4 KiB / 16 KiB per stream 1.85 / 2.95 / 5.38, lz4flex_compress_paged over the same tail ++ add
 *   streams 1.67 / 2.77 / 5.13 (the reopen -- locate, three scan launches, emit, the partial decode, the copy, resume -- costs 5 to 11 %),
 *   re-paging the grown streams from byte 0 14.9 / 16.0 / 18.4; 65 536 x 4 KiB log records in 1 KiB pages appended by 256 B / 1 KiB /
 *   16 KiB 8.89 / 11.5 / 56.3, over tail ++ add 8.34 / 10.9 / 55.5, re-paging 16.0 / 18.6 / 63.1.  Cheaper than re-paging at every size
 *   measured; the gain shrinks as the add outweighs the stream.
 * Not in scope: dictionaries, history, filters, frames; skipping the reopen when the tail page is known to be full; truncation or
 *   in-place overwrite of stream bytes. */
int lz4flex_paged_append(lz4flex_ctx *ctx, const void *add_base, const uint64_t *add_off, const uint32_t *add_len, uint32_t n,
                         uint32_t page_size, uint32_t window_min, uint32_t window_max, uint32_t max_rounds, void *pages,
                         const uint64_t *page_off /* n + 1, entries */, uint32_t *page_len, uint32_t *page_src,
                         uint32_t *n_pages /* in/out */, uint32_t *in_done /* in/out */, int32_t *status, void *stage, uint64_t stage_cap,
                         uint64_t *stage_off /* n, out */, uint32_t *tail_src /* n, out */, void *scratch, uint64_t scratch_cap, void *work,
                         int mem_kind, void *hip_stream);
size_t lz4flex_paged_append_work_size(uint32_t n);
uint64_t lz4flex_paged_append_stage_bound(uint64_t sum_add_len, uint32_t n, uint32_t window_max);

/* Settings (ctx NULL = the default context the scalar / frame entry points use):
 * "compress_mode": 0 = throughput encoder (default; lz4_compress_wave.hip: a valid LZ4 block with this library's own
 *   parse -- any LZ4 decoder returns the input; ratio within a percent of the reference's, usually better), 1 = the
 *   reference's exact bytes (src/block/compress.rs:318-489 restated; about 3x slower).  The scalar calls with a dictionary
 *   (lz4flex_compress_into_with_dict and its _prepend_size_ form) always use the exact encoder; lz4flex_compress_batch_ex follows
 *   this setting.  A Linked frame (src/frame/compress.rs:261-371) written in mode 0 holds blocks whose matches
 *   reach up to 64 KiB back into the blocks before them (LZ4FLEX_BLOCK_HISTORY below: 32 KiB of the stream in front of every
 *   block are its history) -- a dependency-carrying Linked frame that any decoder returns to the input, with a ratio below the
 *   reference's and still one launch per batch of blocks; in mode 1 it holds the reference's bytes (one dependency chain,
 *   milliseconds per block).
 *   2 = high (lz4_compress_high.hip): a deep search for SMALLER blocks, for data that is written once and read many times -- the
 *   decoders cost the same whatever encoder wrote a block.  Every position looks at up to "compress_depth" earlier positions instead of
 *   one, and the parse is lazy by one step.  The bytes are a function of the block and of "compress_depth" ALONE: never of the batch a
 *   block travels in, the device, "compress_subwindows", "compress_deterministic", "compress_sliding_window" or the memory kind.
 *   Where it applies -- every place an independent block without a dictionary is encoded: lz4flex_compress_batch (flag bits 0 and 1
 *   are ignored as in mode 0, and so are the LZ4FLEX_BLOCK_HISTORY bits unless "compress_high_linked" is 1: see there), the scalar
 *   lz4flex_compress_into,
 *   lz4flex_compress_prepend_size and lz4flex_compress_into_with_table (the table is ignored as in mode 0),
 *   lz4flex_compress_batch_packed (its payloads are lz4flex_compress_batch's), and Independent frames through lz4flex_frame_encoder_*,
 *   lz4flex_frame_compress, lz4flex_frame_compress_many and the sharded entry (store-raw rule and checksums unchanged).
 *   Everything else gives MODE 0's bytes under mode 2, decided on the host per call: lz4flex_compress_batch_ex with dict_base,
 *   lz4flex_compress_batch_shared_dict, lz4flex_compress_batch_dict_set, Linked frames; the scalar *_with_dict calls stay exact and
 *   lz4flex_compress_chains is what it is in every mode.  ("compress_high_dict" 1 hands the dictionary calls to mode 2 as well: see
 *   there; "compress_high_linked" 1 does the same for Linked frames and the history bits.)  The OUTPUT_TOO_SMALL rule (out_cap below
 *   get_maximum_output_size: status,
 *   out_len 0, nothing written), LZ4FLEX_MEM_BIG_BLOCKS, the host staging and "MEM_DEVICE calls are asynchronous and allocate nothing"
 *   hold as in mode 0; the kernel's scratch is the context's encoder workspace (not grown), ordered across streams like mode 1's
 *   chain records.
 *   The definition (tests/sim/high_encoder_model.c is the model; the kernel equals it byte for byte).  Positions below 65 536 form
 *   chunk 0 = [0, 65 536) with base 0; a later position p lies in the chunk [p & ~32767, + 32 768) with base = chunk start - 32 768.
 *   Every position p <= n - 12 has the hash (load32(p) * 2654435761u) >> 17; its candidates are the earlier positions q >= base(p)
 *   with the same hash, nearest first, at most "compress_depth" of them (a collision counts).  A candidate matches if its first 4
 *   bytes are equal; its length is counted up to min(chunk end, n - 5) - p; best[p] is the longest match of at least 4 bytes, the
 *   nearest of equal ones.  Parse, from p = 0: best[p].len < 4, or p + 1 in the same chunk with best[p + 1].len > best[p].len: a
 *   literal; otherwise the sequence (literals since the anchor, offset, len) and p += len; the trailing literals close the block.
 *   Sizes in bytes, model == kernel (fast / exact: modes 0 / 1; HCn: liblz4 1.9.3 LZ4_compress_HC at level n; profiles/r16_high_mode.txt):
 *     input                      n     fast    exact  depth 1  depth 4 depth 16 depth 64      HC3      HC9
 *     compression_34k        34308    19373    19888    18537    16926    16335    16125    16255    15894
 *     compression_65k        64723    36493    37150    34053    31186    29926    29549    29849    29086
 *     compression_66k_JSON   66675    15216    15268    15574    13257    12843    12390    12542    12213
 *     JSON tile              65536    14955    15033    15320    13035    12629    12181    12339    12029
 *     log, 64 KiB            65536    19850    19908    19302    17957    17154    16780    17057    16409
 *     log, 4 KiB              4096     1595     1575     1568     1501     1481     1473     1479     1474
 *     log, 1 MiB           1048576   308925   309864   296949   274912   259570   252256   255599   239996
 *     JSON x 4, 200 000     200000    44689    44837    45452    38370    37055    35495    35346    33361
 *     zeros                 100000      407      404      409      409      409      409      403      403
 *   Depth 16 is 6 % to 35 % below min(fast, exact) on every compressible item and within 2.4 % of HC level 3; random bytes are the
 *   same 70 276 in every column; runs of one byte are a few bytes above mode 0 (a chunk end splits the run).
 *   Time: MI355X, device-resident batches, ms per lz4flex_compress_batch call, one session (tools/high_bench.py), as mode 0 / mode 1 /
 *   mode 2 at depth 4, 16, 64 (liblz4 HC level 3 / 9 on 16 host threads over the same blocks): 16 384 x 64 KiB JSON tiles 3.1 / 18.3
 *   / 68 / 124 / 284 (HC 234 / 764), ratio 0.230 / 0.232 / 0.200 / 0.193 / 0.186 (HC 0.189 / 0.183); 65 536 x 4 KiB log records 6.3
 *   / 5.8 / 30 / 45 / 59 (HC 663 / 820), ratio 0.391 / 0.393 / 0.370 / 0.361 / 0.360 (HC 0.362 / 0.360); 256 x 4 MiB log blocks 4.5
 *   / 284 / 114 / 240 / 649 (HC 357 / 1 481), ratio 0.294 / 0.295 / 0.262 / 0.247 / 0.240 (HC 0.243 / 0.228) -- depth 16 costs 40 x
 *   mode 0 on the tiles and is 1.9 x ahead of 16 CPU threads at HC level 3 there, 15 x on the records, 1.5 x on the 4 MiB blocks (a
 *   block's chunks are serial in one workgroup); every block was decoded by the oracle's decoder
 *   Environment: LZ4FLEX_COMPRESS_MODE=exact|fast|high (or 1|0|2).
 * "compress_depth" ("compress_mode" 2 alone reads it): the candidates examined per position, 1 ... 256, default 16.  Encode time
 *   grows with it, the blocks shrink (table above); the decoders do not care.
 * "compress_parse" ("compress_mode" 2 alone reads it; modes 0 and 1 ignore it): 0 (default) = the one-step lazy parse of the definition
 *   above.  1 = the optimal parse: candidates and best[] are unchanged (with a dictionary or a history: the dictionary form's), and a
 *   backward pass chooses HOW MUCH of best[p] to take.  Per chunk, in segments of S = 2 048 positions that know nothing of each other
 *   (j relative to the chunk's start, cn = its positions that exist, ext(v) = v < 15 ? 0 : (v - 15) / 255 + 1), for j = cn - 1 down to 0:
 *   se = min((j / S + 1) * S, cn), CO(x) = x >= se ? 0 : cost[x]; L = best[j].len, c = infinity, pick = 0; if L >= 4: Lp = min(L, se - j),
 *   c = 3 + ext(Lp < 4 ? 0 : Lp - 4) + CO(j + L), pick = L, and for l = min(L - 1, 35, se - j) down to 4: v = 3 + ext(l - 4) + CO(j + l),
 *   v < c: c = v, pick = l; then 1 + CO(j + 1) < c: c = 1 + CO(j + 1), pick = 0; cost[j] = c, len'[j] = pick.  The walk reads len'[] in
 *   best[].len's place, a literal is len'[j] < 4 (no lazy test), offsets are best[].off.  Ties: the full length, then the longer short
 *   length, the literal last; a literal run's own length bytes are not priced.  A shortened match ends where a full one could, so the
 *   end-of-block rules hold as before.  The definition is tests/sim/high_optimal_model.c, the kernel equals it byte for byte, in all
 *   three forms (plain, "compress_high_dict", "compress_high_linked") and through every entry that reaches them.  Blocks are 1.6 % to
 *   3.4 % smaller on text, JSON and log records at depths 4, 16 and 64; on run-heavy data a block may be a few bytes LARGER than under
 *   parse 0 -- nothing is promised there.  Environment: LZ4FLEX_HIGH_PARSE=optimal|lazy (or 1|0).
 * "compress_high_dict" ("compress_mode" 2 alone reads it): 0 (default) = calls with dictionaries give mode 0's bytes, as above.  1 =
 *   they take the high encoder's dictionary form: lz4flex_compress_batch_ex with dict_base, lz4flex_compress_batch_shared_dict,
 *   lz4flex_compress_batch_dict_set, lz4flex_compress_into_with_dict and lz4flex_compress_prepend_size_with_dict.  The blocks are
 *   ordinary dictionary blocks: lz4flex_decompress_batch_shared_dict, _dict_set, _ex and their partial forms read them as they read
 *   any other.  Kept: the OUTPUT_TOO_SMALL rule; _ex: a block with a dictionary and flags[i] != 0 gets LZ4FLEX_E_INVALID_ARG, out_len
 *   0, nothing written; sets: id 0xFFFFFFFF = no dictionary, an id >= K is refused in the same way; a block without a dictionary, or
 *   with one of less than 4 bytes, gets mode 2's plain bytes (mixed batches included); MEM_HOST stages as in mode 0, MEM_DEVICE calls
 *   allocate nothing; dictionaries may overlap each other and the inputs; Linked frames keep mode 0's bytes ("compress_high_linked").  The shared entry
 *   prepares its one dictionary once per call ("compress_high_digest" below).
 *   The definition (tests/sim/high_dict_model.c; the kernel equals it byte for byte -- a function of block, dictionary and
 *   "compress_depth" alone).  H = dict_len < 4 ? 0 : min(dict_len, 32 768); H == 0: the plain definition above.  Otherwise the stream
 *   is S = [the dictionary's last H bytes | block] and EVERY chunk is 32 KiB: chunk c = block positions [c * 32 768, + 32 768), its
 *   base 32 768 positions earlier in S and not below S's first byte -- chunk 0 sees the dictionary's tail and itself, every later
 *   chunk the block alone; an offset is at most 65 535 (65 532 in practice).  Hashed positions: the block's p <= n - 12 and the
 *   tail's q with q + 4 <= H (the three positions whose 4 bytes straddle the dictionary's end are never candidates: the dictionary's
 *   order is a function of the dictionary alone).  Candidates, best[] and the parse are the plain definition's, lengths counted over
 *   S (a match may start in the dictionary and run on into the block) up to min(chunk end, n - 5) - p; n < 12: literals only.
 *   Sizes at depth 16 (no dictionary -> with it; oracle = the reference's compress_with_dict): a 4 KiB JSON record against a 32 KiB
 *   dictionary 1 145 -> 604 (oracle 780), a 4 KiB text record 2 787 -> 1 799 (oracle 2 409); over 24 (block, dictionary) cases of
 *   the two fixtures 65 502 -> 54 767 (oracle 67 576).
 *   Measured: MI355X, device-resident batches against one 32 KiB dictionary, one session with the legs alternating
 *   (tools/high_dict_bench.py, profiles/r17_high_dict.txt), ms per call and ratio; every block decoded by the oracle's decoder.
 *   65 536 x 4 KiB log records: mode 0 with the dictionary 5.6 ms, 0.298; mode 1 with it 57.6, 0.315; mode 2 with it through
 *   lz4flex_compress_batch_shared_dict at depth 4 / 16 / 64: 29.5 / 52.8 / 132 ms, 0.2705 / 0.2554 / 0.2499 (with
 *   "compress_high_digest" 0 and through lz4flex_compress_batch_ex: 86 / 136 / 252 ms, the same bytes); mode 2 at depth 16 without a
 *   dictionary 44.8 ms, 0.361.  16 384 x 64 KiB JSON tiles: mode 0 with the dictionary 5.0 ms, 0.200; mode 1 with it 67.4, 0.163;
 *   mode 2 with it 607 / 1 178 / 1 985 ms, 0.1547 / 0.1478 / 0.1414 (digest 0 and _ex: 643 / 1 239 / 2 040); mode 2 at depth 16
 *   without a dictionary 124 ms, 0.193.  The tiles' dictionary is a piece of the file the tiles repeat: most positions of chunk 0
 *   find a match that runs to the chunk's end, and counting it (up to 32 KiB per position) is what the ten-fold time goes to -- the
 *   plain form's known cost on runs, met on real data; the digest saves only the sort there.  (Read off the data's shape and the
 *   digest's small gain, not profiled.)
 *   Environment: LZ4FLEX_HIGH_DICT=1.
 * "compress_high_linked" ("compress_mode" 2 alone reads it): 0 (default) = the LZ4FLEX_BLOCK_HISTORY bits are ignored and Linked
 *   frames are written by the throughput encoder, as above.  1 = a block with h = flags[i] >> 8 bytes of its stream in front of it is
 *   encoded by the high encoder's dictionary form with those bytes as its dictionary: block i gets exactly the bytes
 *   tests/sim/high_dict_model.c gives (block, in_base[in_off[i] - h .. in_off[i]), "compress_depth") -- the bytes lz4flex_compress_batch_ex
 *   gives the block under "compress_high_dict" 1 with the h bytes passed as its dictionary.  So: the last H = min(h, 32 768) bytes are
 *   chunk 0's history and every chunk is 32 KiB; the three positions whose 4 bytes straddle the block's start are not hashed; h < 4
 *   gives the plain definition's bytes, and so does a block of a history batch with h == 0 (flag bits 0 and 1 are ignored as ever;
 *   blocks with and without history mix freely in one launch).  The bytes are a function of the block, the at most 32 KiB in front of
 *   it and "compress_depth" alone -- never of the batch, the memory kind, the number of streams or how a stream was cut into write()
 *   calls.  Where it applies: lz4flex_compress_batch with a flags array (one launch for all blocks: the history is input;
 *   lz4flex_compress_batch_packed follows lz4flex_compress_batch, but carries no flag words and so no history), and Linked frames through lz4flex_frame_encoder_*, lz4flex_frame_compress and
 *   lz4flex_frame_compress_many (one launch over all blocks of all streams; flags, the 32 KiB kept between write() calls, the
 *   store-raw rule and the checksums are mode 0's).  Unchanged: lz4flex_compress_batch_ex (a block with a dictionary and flags[i] != 0
 *   is still refused), "compress_mode" 0 and 1, Independent frames, lz4flex_compress_chains, the sharded entry (Linked frames do not
 *   shard).  MEM_HOST stages the bytes in front of a block with it and refuses h > in_off[i], as in mode 0.  No read leaves the
 *   aligned dwords that hold [in - H, in + n).  A history longer than 32 KiB is not used: the window is 64 KiB of LDS with 16-bit
 *   positions.
 *   Sizes at depth 16, payload bytes, independent -> linked (the model; the kernel equals it): 1 MiB of log in 64 KiB blocks 274 737
 *   -> 259 660 (depth 4: 288 883 -> 275 002, depth 64: 268 474 -> 252 346; mode 0's Linked frame: about 0.29 of the input, 0.248
 *   here); the text fixture in 16 KiB pieces 35 274 -> 30 192.
 *   Measured: MI355X, device-resident, 1 GiB per shape, one session with the legs alternating (tools/high_linked_bench.py,
 *   profiles/r18_high_linked.txt), every frame decoded by the oracle; ms per call and ratio as mode 0 Linked | mode 2 Independent at
 *   depth 4 / 16 / 64 | mode 2 Linked at depth 4 / 16 / 64.  256 streams x 4 MiB of log in 64 KiB blocks through
 *   lz4flex_frame_compress_many: 5.4, 0.2932 | 84 / 198 / 546, 0.2754 / 0.2620 / 0.2560 | 114 / 243 / 653, 0.2616 / 0.2468 / 0.2399 (a
 *   64 KiB block with history is two 64 KiB windows instead of one); 4 096 streams x 256 KiB: 6.2, 0.2956 | 85 / 199 / 548 | 114 /
 *   244 / 655, 0.2649 / 0.2505 / 0.2437; blocks of 4 MiB (one per stream): the same bytes and times with the setting on and off.  A
 *   raw batch of 16 384 x 64 KiB JSON tiles, each behind 32 KiB of the tile in front: 4.7, 0.2199 | 68 / 123 / 283, 0.1999 / 0.1931 /
 *   0.1857 | 113 / 211 / 472, 0.1878 / 0.1801 / 0.1715.
 *   Environment: LZ4FLEX_HIGH_LINKED=1.
 * "compress_high_digest" (the dictionary form of "compress_mode" 2, lz4flex_compress_batch_shared_dict alone): 1 (default) = a
 *   kernel in front of the encoder sorts the dictionary tail's hashed positions ONCE per call (128 KiB in the encoder's workspace:
 *   u16 sorted[H - 3] and the bucket bounds u16 start[32 769]); a block then sorts its own positions only, and a position's
 *   candidates are its left neighbours of equal hash in its own order, then the digest's bucket from its end downwards -- nearest
 *   first across both, the same count and the same stop: the same bytes.  0 = every block sorts the tail's positions with its own,
 *   which is what lz4flex_compress_batch_ex and lz4flex_compress_batch_dict_set always do (a digest per dictionary of a set is not
 *   kept yet).
 * "compress_sliding_window" (throughput encoder): how far the 64 KiB windows of a block LONGER than 64 KiB advance.  2 (default
 *   since round 5) = by 48 KiB, so every window start has 16 ... 64 KiB of the block behind it -- the reference's window slides
 *   continuously (src/block/compress.rs:403-405); 4 MiB log blocks: ratio 0.2940 (the reference: 0.2947) for a third more indexing;
 *   1 = by 32 KiB (round 4's default: 0.2929, every byte indexed twice); 0 = by 64 KiB (0.3027, fastest, round 3's bytes).
 *   Blocks of <= 64 KiB are one window either way.  Environment: LZ4FLEX_SLIDING_WINDOW=0|1|2.
 * "compress_subwindows" (throughput encoder): 0 (default) = by batch size -- a batch that leaves most of the encoder's persistent
 *   workgroups ("compress_workgroups", read-only: two per CU) without a block cuts every block of at most 64 KiB into 4 (n * 4 <=
 *   workgroups), 3 or 2 sub-windows that different workgroups encode side by side: a scalar compress_into and small batches take
 *   about half the time, at a ratio a few tenths of a percent higher; the BYTES of a block therefore depend on the size of the batch
 *   it travels in (always a valid block) and on the device's CU count; 1 = never, 2 / 3 / 4 = always.
 * "compress_deterministic": 1 = the bytes of a block are a function of the block and of the settings above alone -- never of the batch
 *   it travels in or of the device ("compress_subwindows" is taken as 1; small batches and the scalar compress_into then cost about twice
 *   the time).  What a caller sets that stores, hashes, deduplicates or golden-files compressed blocks (src/block/compress.rs:599-601
 *   is a pure function of its input; "compress_mode" 1 is the one that also gives the REFERENCE's bytes).  0 (default).
 * Kernel selection, for measurements only (every choice produces the same bytes / lengths / error variants):
 * "decompress_variant": 0 = by batch size (default), 7 = one block per WORKGROUP, token chain and copies parallel inside the
 *   block (lz4_decompress_pcd.hip: few, large blocks; 8 = the same with its small test geometry, 10 / 11 = with 256 / 512 lanes
 *   per block: what 0 picks for 513 ... 640 / 257 ... 512 blocks), 13 = one block per WAVEFRONT, one lane per sequence
 *   (lz4_decompress_seq.hip, round 6: what 0 picks for 641 ... 14 336 blocks; it replaced 5 / 6, the wave decoder and its
 *   two-wavefront form, which are gone), 4 = parser / copier split decoder (larger batches), 12 = the split decoder's parser feeding
 *   a piece cutter and the replay decoder's copy engine inside one workgroup (lz4_decompress_fused.hip: level with 4 on JSON, ahead on
 *   text, behind on incompressible data and runs; -DLZ4FLEX_TOOLS builds only since round 6), 9 = plan / replay
 *   (lz4_decompress_plan.hip + lz4_decompress_replay.hip; -DLZ4FLEX_TOOLS builds only since round 5: slower than 0 on every shape
 *   measured), 1 = decoder whose window lives in HBM/L2 (always used for dictionary blocks; prefix blocks without a dictionary go to 7, or
 *   to 13 when 13 is pinned or picked and the batch is not chained); "decompress_blocks_per_wg" (variant 4: 0 = 64, the default at every batch size; 8/16/32: the older narrow geometries, tests); "decompress_lanes"
 *   (16; 8/32/64 in -DLZ4FLEX_ALL_VARIANTS builds, variant 1); exact encoder: "compress_lanes" (8/16 lanes of a wavefront per
 *   block), "compress_variant" (1 = group encoder + emitter wavefront; 3 = group encoder alone, -DLZ4FLEX_ALL_VARIANTS builds);
 *   "decompress_second_pass" (tests: 0 leaves the blocks that variants 7 ... 13 hand to the reference-order kernel marked with
 *   status 0x7F000001 instead of decoding them again); "decompress_pcd_pair" (variants 7 / 8: 1 = batches of at most 128 LARGE
 *   blocks get a parser and a copier workgroup per block -- parse and copy of a block overlap, a single huge block uses two
 *   CUs' worth of time instead of one; 0 = never; 2 = every batch of at most 128 blocks: tests); "compress_carry_wait" (tests: 0 = a 64 KiB window of the throughput
 *   encoder that has to wait for the window before it -- few, large blocks: a block's windows run on different workgroups --
 *   gives up at once instead of after a fraction of a second; such a block is encoded again by the launch that follows, to
 *   the same bytes: a time-sliced GPU costs time, never an error); "decompress_level_chains" (default 1024; lz4flex_frame_decompress_many:
 *   a call that holds at least this many Linked streams decodes block k of every stream in ONE launch -- a plain batch whose prefixes
 *   the launches before it have written -- instead of a workgroup per block that polls its predecessor: thousands of short streams,
 *   4 096 x 256 KiB 6.7 -> 3.1 ms per GiB; 0 = never; tests set 1); "compress_shared_dict" (see lz4flex_compress_batch_shared_dict);
 *   "decompress_shared_dict" (see lz4flex_decompress_batch_shared_dict); "decompress_partial" (see lz4flex_decompress_batch_partial);
 *   "frame_range_pass_bytes" and "frame_range_checksums" (see lz4flex_frame_read_ranges); "fit_serial" (see the fit batches);
 *   "packed_scan_tile" (read-only: the sizes one workgroup of the packed entries' offset scan takes, see the packed batches).
 * Keys that start with "debug_" inject faults for this library's own tests; they are unsupported and refused
 * (-LZ4FLEX_E_INVALID_ARG) unless the process runs with LZ4FLEX_TEST_HOOKS=1.  "debug_exact_dict_piece" (set only; a count, 0 = no
 * limit): "compress_mode" 1 calls with dictionaries build their chain records in pieces of at most that many blocks.
 * The key is looked at before a context is: an unknown key and a refused "debug_" key answer -LZ4FLEX_E_INVALID_ARG on any machine,
 * a known key with ctx NULL needs the default context and with it a device (-LZ4FLEX_E_NO_DEVICE without one).  The same for
 * lz4flex_get_tuning. */
int lz4flex_set_tuning(lz4flex_ctx *ctx, const char *key, int value);
/* the current value of a setting (>= 0), or -LZ4FLEX_E_INVALID_ARG for an unknown key.  Two read-only lists need no device and no
 * context: "dispatch_threshold_<i>" (the batch sizes at which the default decoder dispatch changes kernel or geometry, ascending) and
 * "decoder_config_<i>" (every decoder configuration this build can be pinned to: variant * 1000 + "decompress_lanes" (variant 1) /
 * "decompress_blocks_per_wg" (variant 4) / 0); both end where the key is refused */
int lz4flex_get_tuning(lz4flex_ctx *ctx, const char *key);

/* ---- frame (src/frame/) ------------------------------------------------------------------ */
typedef struct lz4flex_frame_info {   /* frame::FrameInfo, src/frame/header.rs:130-149 */
    int32_t has_content_size;
    uint64_t content_size;
    int32_t block_size;       /* frame::BlockSize: 0 Auto, 4 Max64KB, 5 Max256KB, 6 Max1MB, 7 Max4MB, 8 Max8MB */
    int32_t block_mode;       /* frame::BlockMode: 0 Independent, 1 Linked */
    int32_t block_checksums;
    int32_t content_checksum;
    int32_t legacy_frame;
} lz4flex_frame_info;

/* io::Write / io::Read stand-ins: return bytes written/read, or < 0 for an I/O error */
typedef int64_t (*lz4flex_write_fn)(void *user, const uint8_t *buf, size_t len);
typedef int64_t (*lz4flex_read_fn)(void *user, uint8_t *buf, size_t len);

typedef struct lz4flex_frame_encoder lz4flex_frame_encoder;
/* FrameEncoder::with_frame_info, src/frame/compress.rs:133-151 (info NULL => FrameEncoder::new) */
lz4flex_frame_encoder *lz4flex_frame_encoder_new(const lz4flex_frame_info *info, lz4flex_write_fn w, void *user);
/* io::Write::write, :375-396 */
int64_t lz4flex_frame_encoder_write(lz4flex_frame_encoder *e, const uint8_t *buf, size_t len);
/* io::Write::flush, :398-403 */
int lz4flex_frame_encoder_flush(lz4flex_frame_encoder *e);
/* try_finish, :173-187 */
int lz4flex_frame_encoder_try_finish(lz4flex_frame_encoder *e, lz4flex_err_detail *detail);
/* frame_info(), :159-161 */
void lz4flex_frame_encoder_frame_info(lz4flex_frame_encoder *e, lz4flex_frame_info *out);
/* how many uncompressed bytes the encoder gathers per kernel launch (default 64 MiB); before the first write */
int lz4flex_frame_encoder_set_batch_bytes(lz4flex_frame_encoder *e, size_t bytes);
void lz4flex_frame_encoder_free(lz4flex_frame_encoder *e);

typedef struct lz4flex_frame_decoder lz4flex_frame_decoder;
/* FrameDecoder::new, src/frame/decompress.rs:76-89 */
lz4flex_frame_decoder *lz4flex_frame_decoder_new(lz4flex_read_fn r, void *user);
/* io::Read::read, :353-367: bytes read, 0 at end of frame / EOF, < 0 = -code */
int64_t lz4flex_frame_decoder_read(lz4flex_frame_decoder *d, uint8_t *buf, size_t len, lz4flex_err_detail *detail);
/* io::BufRead::fill_buf, :410-416: *buf = the decoded bytes not consumed yet (valid until the next call on this decoder),
 * return value = their count; decodes the next batch of blocks when there are none; 0 at end of frame / EOF, < 0 = -code */
int64_t lz4flex_frame_decoder_fill_buf(lz4flex_frame_decoder *d, const uint8_t **buf, lz4flex_err_detail *detail);
/* io::BufRead::consume, :418-421; amt must not exceed what the last fill_buf returned (the reference asserts) */
int lz4flex_frame_decoder_consume(lz4flex_frame_decoder *d, size_t amt);
int lz4flex_frame_decoder_set_batch_bytes(lz4flex_frame_decoder *d, size_t bytes);
void lz4flex_frame_decoder_free(lz4flex_frame_decoder *d);

/* One-shot helpers over flat host buffers: FrameEncoder::with_frame_info + write_all + finish,
 * and FrameDecoder::new + read_to_end (first frame only; *consumed = input bytes read -- on success where the reference's reader
 * stands: behind the EndMark and content checksum, at the end of a cut input, or behind the empty block that ended the reading). */
int64_t lz4flex_frame_compress(const uint8_t *in, size_t in_len, const lz4flex_frame_info *info,
                               uint8_t *out, size_t out_cap, lz4flex_err_detail *detail);
int64_t lz4flex_frame_decompress(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap,
                                 size_t *consumed, lz4flex_err_detail *detail);
/* worst-case frame size for `in_len` bytes under `info` (header + per-block overhead + EndMark) */
size_t lz4flex_frame_compress_bound(size_t in_len, const lz4flex_frame_info *info);
/* frame::FrameInfo::write / read, src/frame/header.rs:232-373 */
int64_t lz4flex_frame_info_write(const lz4flex_frame_info *info, uint8_t *out, size_t out_cap);
int64_t lz4flex_frame_info_read(const uint8_t *in, size_t in_len, lz4flex_frame_info *info,
                                lz4flex_err_detail *detail);
/* XXH32 as used by the frame format (twox-hash in the reference); host */
uint32_t lz4flex_xxh32(const uint8_t *data, size_t len, uint32_t seed);
/* batched XXH32 of n DEVICE-resident buffers base[off[i] .. +len[i]) -> out[i] (device), on hip_stream: the block
 * checksums of src/frame/compress.rs:313-316 / src/frame/decompress.rs:178-187 for device-resident frames */
int lz4flex_xxh32_batch_device(const void *base, const uint64_t *off, const uint32_t *len, uint32_t n, uint32_t seed,
                               uint32_t *out, void *hip_stream);

/* ---- frame segments on the device (multi-GPU frame path: every rank assembles the segment of its block range) ---------
 * What FrameEncoder::write_block does around the codec call for each block (src/frame/compress.rs:282-316): the 4-byte
 * BlockInfo (frame/header.rs:108-124), the store-raw rule (compress.rs:301-306: a block that did not shrink is stored
 * uncompressed, high bit set), the payload and the optional XXH32 of the payload -- for n blocks already compressed by
 * lz4flex_compress_batch (MEM_DEVICE), back to back into `seg`.  Every pointer is device memory, the work is enqueued
 * on hip_stream.  seg_off: n + 1 u64, filled with each block's offset in seg and, last, the bytes written (read it
 * back to size the exchange).  seg must hold sum(in_len) + 8 n bytes.  scratch: 16 n bytes, needed with
 * block_checksums only. */
int lz4flex_frame_assemble_device(const void *src_base, const uint64_t *src_off, const uint32_t *in_len,
                                  const void *comp_base, const uint64_t *comp_off, const uint32_t *comp_len, uint32_t n,
                                  int block_checksums, void *seg, uint64_t *seg_off, void *scratch, void *hip_stream);
/* n independent byte ranges src_base[src_off[i] .. +len[i]) -> dst_base[dst_off[i] ..) in one launch (decode side: blocks
 * stored raw go straight to their place in the output, src/frame/decompress.rs:262-271) */
int lz4flex_copy_batch_device(const void *src_base, const uint64_t *src_off, const uint32_t *len, void *dst_base,
                              const uint64_t *dst_off, uint32_t n, void *hip_stream);

/* The block-header walk of FrameDecoder::read_block (src/frame/decompress.rs:231-247) for a frame in DEVICE memory: follows
 * the BlockInfo words from header_len to the EndMark and writes, per block, the payload offset and the length word (high
 * bit = stored uncompressed).  info (4 x u32, device): [0] blocks found, [1] 0 ok / 1 truncated frame / 2 BlockTooBig
 * (a block longer than block_size, :242-247) / 3 more than max_blocks, [2..3] offset behind the EndMark.  Only the few
 * result words travel to the host; the frame stays where it is. */
int lz4flex_frame_walk_device(const void *frame, uint64_t frame_len, uint32_t header_len, int block_checksums, uint32_t block_size,
                              uint32_t max_blocks, uint64_t *payload_off, uint32_t *len_word, uint32_t *info, void *hip_stream);

/* ---- many frames at once (BASELINE configs[4] in the shape that has parallelism in it: N streams, a frame each) ------------------
 * What N FrameEncoders / FrameDecoders do, one per stream (src/frame/compress.rs:261-371, src/frame/decompress.rs:189-342), as ONE
 * batch: the blocks of all streams are encoded by one launch; on the way back the BlockInfo words of all frames are walked on the
 * device (a thread per frame) and all blocks are decoded by one launch -- for BlockMode::Linked frames a chained batch of N chains
 * that advance together (src/frame/decompress.rs:195-222: a Linked frame is a dependency chain; one stream is serial, N streams are
 * N-fold parallel).  Stream i is in_base[in_off[i] .. + in_len[i]) and its result goes to out_base[out_off[i] .. + out_cap[i]);
 * out_len[i] = bytes written, status[i] = 0 or the negative code lz4flex_frame_compress / lz4flex_frame_decompress would have
 * returned for that stream alone (detail: nullable, n entries).  in_off / in_len / out_off / out_cap / out_len / status / detail
 * are HOST arrays; in_base / out_base are DEVICE memory (LZ4FLEX_MEM_DEVICE: work on hip_stream) or HOST memory (LZ4FLEX_MEM_HOST:
 * staged through the context's scratch; hip_stream ignored).  The calls BLOCK: they return after the work has completed (they synchronise
 * hip_stream), and they may allocate: the context's scratch grows with the largest job seen (hipMalloc / hipFree, a device-wide
 * synchronisation, whenever a larger one arrives).  The scratch lives on the CONTEXT's device whatever the calling thread's current one is.
 * compress_many: info NULL = FrameInfo::default(); BlockSize::Auto is resolved per stream from its length (frame/header.rs:57-67);
 * has_content_size: every frame's header carries ITS stream's length (info->content_size is not read).  compress_mode fast: the
 * frames hold this library's own parse (a Linked frame's blocks reach into the 32 KiB in front of them); exact: the reference's
 * bytes (Linked: lz4flex_compress_chains, a chain per stream).  out_cap[i] >= lz4flex_frame_compress_bound(in_len[i], info) always fits.
 * decompress_many: out_cap[i] should be the stream's size or little more (a frame's block table is sized from it).  The batch takes
 * frames whose blocks all fill the block size but the last; anything else (skippable frames, flush() boundaries,
 * checksum mismatches, corrupt blocks, buffers too small, legacy frames) is decoded by lz4flex_frame_decompress, stream by stream,
 * which also names the error -- same results, one stream's speed.  A stream's FIRST frame is decoded; bytes behind it are not read
 * (FrameDecoder::read returns 0 at the end of a frame, tests/tests.rs:633-647). */
int lz4flex_frame_compress_many(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint64_t *in_len, uint32_t n,
                                const lz4flex_frame_info *info, void *out_base, const uint64_t *out_off, const uint64_t *out_cap,
                                uint64_t *out_len, int32_t *status, int mem_kind, void *hip_stream);
int lz4flex_frame_decompress_many(lz4flex_ctx *ctx, const void *in_base, const uint64_t *in_off, const uint64_t *in_len, uint32_t n,
                                  void *out_base, const uint64_t *out_off, const uint64_t *out_cap, uint64_t *out_len, int32_t *status,
                                  lz4flex_err_detail *detail, int mem_kind, void *hip_stream);

/* ---- seekable frames: a block index and batched byte-range reads -----------------------------------------------------------------
 * Every other frame entry decodes a frame from its first byte to its last (the reference's FrameDecoder has no other way,
 * src/frame/decompress.rs:189-342).  The blocks of a BlockMode::Independent frame do not need each other, so a table of where each
 * block lies and which content bytes it holds is enough to decode only the blocks a byte range touches.
 * lz4flex_frame_index_create indexes the FIRST frame of frame[0 .. frame_len) (mem_kind LZ4FLEX_MEM_HOST: staged through the context's
 *   scratch once; LZ4FLEX_MEM_DEVICE: read where it is): the header is parsed on the host (lz4flex_frame_info_read), the BlockInfo words
 *   are walked on the device (one thread, as lz4flex_frame_walk_device), the decoded size of every compressed block comes from the size
 *   scan of lz4flex_decompressed_size_batch (nothing is decoded; a stored block's size is its length) and the content offsets from the
 *   packed entries' offset scan.  The index holds, in device memory it owns and in a host copy: content_off[0 .. blocks] (exclusive
 *   sums of the decoded sizes; content_off[blocks] = the content size), payload_off[b] (of block b's payload in the frame) and
 *   len_word[b] (its BlockInfo word: the payload's length, high bit = stored); and the frame info, the content size and frame_bytes,
 *   the offset behind the EndMark and the content checksum (where a second frame would start; bytes behind it are not read).  Like a
 *   dictionary set it belongs to the context's DEVICE: any context of that device may read through it, nothing in it is written after
 *   create, it may be freed before or after the context.  create blocks until the index is ready; the frame may be freed or moved
 *   afterwards -- lz4flex_frame_read_ranges takes the frame again.
 *   An index exists only for a structurally sound frame: create returns the negative code, and fills detail, as
 *   lz4flex_frame_decompress does for the same bytes when no checksum is wrong -- the earliest defect in stream order: the header's
 *   errors (wrong magic, header checksum, reserved bits, block size, version, dictionary id, a skippable frame first); a compressed
 *   block that does not scan or decodes to more than the block size, in front of where the walk stopped (that one block is decoded
 *   once, with a sink of the block size: -LZ4FLEX_FE_DECOMPRESSION, detail = the decoder's inner / expected / actual); a truncated
 *   frame (-LZ4FLEX_FE_IO; also one that ends where its EndMark should be, which a streaming reader takes for "no more bytes yet",
 *   src/frame/decompress.rs:231-238) or -LZ4FLEX_FE_BLOCK_TOO_BIG where the walk stopped; -LZ4FLEX_FE_CONTENT_LENGTH when the header's content
 *   size is not content_off[blocks].  A sound block of no bytes at all (a stored block of length 0, a compressed block that decodes to
 *   nothing) ends the index as it ends the reader's read_to_end (src/frame/decompress.rs:344-349): the blocks in front of it are the
 *   index, frame_bytes is the offset behind it, and neither the content size nor anything behind it is looked at.  (_info is the
 *   header's FrameInfo verbatim in every case: its content_size and content_checksum say what the header says, not what such an index holds.)
 *   NO CHECKSUM IS LOOKED AT by create.  -LZ4FLEX_E_UNSUPPORTED: BlockMode::Linked frames (a block
 *   needs the 64 KiB in front of it, transitively: there is nothing to seek in) and legacy frames.  -LZ4FLEX_E_INVALID_ARG: out or
 *   frame NULL, a mem_kind other than HOST / DEVICE (checked before a context is looked at); -LZ4FLEX_E_NO_DEVICE without a device.
 *   _table copies the host tables out (blocks + 1, blocks, blocks entries; any pointer may be NULL).
 * lz4flex_frame_read_ranges reads m ranges: range r is content bytes [range_off[r], range_off[r] + range_len[r]).  With S the content
 *   size: out_len[r] = min(range_len[r], S - range_off[r]), 0 for range_off[r] >= S (clipped like a read at end of file, status 0); those
 *   bytes -- what a full decode of the frame has at that position -- are written at out_base + out_off[r].  Nothing is written in front
 *   of out_base + out_off[r] or at or behind out_base + out_off[r] + out_len[r]: strict, as for lz4flex_decompress_batch_partial.
 *   Ranges whose output regions overlap are the caller's error.  range_off / range_len / out_off / out_len / status / detail
 *   (nullable, m entries) are HOST arrays; frame and out_base are both DEVICE memory (LZ4FLEX_MEM_DEVICE: work on hip_stream) or both
 *   HOST memory (LZ4FLEX_MEM_HOST: per range ONE copy of the frame span from its first touched block's BlockInfo word to the end of its
 *   last one goes up -- a small read uploads only the blocks it touches -- and its bytes come back).  The call BLOCKS until the work is
 *   done and may grow the context's scratch, as the *_many calls do.
 *   Errors are per range: status[r] = -LZ4FLEX_FE_BLOCK_CHECKSUM when the stored XXH32 of a touched block does not match its payload
 *   (frames with block checksums, stored blocks too; the payload is hashed WHOLE, also when one byte of the block is wanted; setting
 *   "frame_range_checksums", default 1: 0 skips this); -LZ4FLEX_FE_DECOMPRESSION with detail[r].inner when a touched block does not
 *   decode up to its last wanted byte, e.g. because the frame changed since create (a block that decodes without an error but to fewer
 *   bytes than the index says: inner 0, expected / actual = the bytes wanted / produced).  Among several defects the first block in
 *   stream order decides, within a block the checksum before the decode (the reference's order).  On error out_len[r] = 0 and the
 *   range's own output region may hold anything; the other ranges are unaffected.
 *   NOT VERIFIED: the content checksum, by neither call (a range read does not see the whole content); block checksums of blocks no range
 *   touches; anything about a frame that differs from the one the index was made from beyond what the touched blocks show.
 *   What a read launches: the host locates each range in the host tables (csrc/frame_range.h: binary search) and sends one 64-byte record per
 *   range; frame_range_plan_kernel (a thread per touched block) writes the items of two lz4flex_decompress_batch_partial batches -- every
 *   touched compressed block from its first byte up to the range's last byte in it, straight into out_base; a range's first block when
 *   the range starts inside it (a "head") into scratch -- and of two copy batches (stored blocks' spans from the frame, heads' spans from
 *   scratch); XXH32 + compare over the touched payloads; frame_range_verdict_kernel (a wavefront per range) folds the items' results
 *   into the m verdicts that come back.  Many ranges that hit the same block decode it once each.  The ranges are cut into passes whose
 *   scratch (heads; MEM_HOST: staged spans and outputs too) stays under the setting "frame_range_pass_bytes" (default 256 MiB; a pass
 *   takes at least one range).  "decompress_partial" picks the partial decoder as for lz4flex_decompress_batch_partial.
 *   Measured once on an MI355X (tools/frame_range_bench.py, one session, profiles/r14_frame_index.txt; 1 GiB of content, device-resident,
 *     ms per blocking call): 16 384 blocks of 64 KiB JSON -- create 10.5 (the one-thread walk 6.1, the size scan 0.6); one range of 1 MiB
 *     0.70, 16 of them 0.71, 1 024 ranges of 4 KiB 0.58, 65 536 of them 15.2 (nearly every one a head), the whole content as one range
 *     2.07; lz4flex_frame_decompress_many of the same frame 8.75.  With block checksums: 16 x 1 MiB 1.10, "frame_range_checksums" 0: 0.70.
 *     256 blocks of 4 MiB log lines -- create 6.4 (the size scan 6.1); one range of 1 MiB 10.1 against 5.0 for the full decode: NOT
 *     cheaper -- a range that starts inside a 4 MiB block decodes it from its first byte with one wavefront (the time is the head's
 *     partial-decode launch); 65 536 ranges of 4 KiB there take 7.7 s.  Random access pays off on frames of small blocks.
 *   Call-level returns: -LZ4FLEX_E_INVALID_ARG for x == NULL or a mem_kind other than HOST / DEVICE; m == 0 returns 0; then
 *   -LZ4FLEX_E_INVALID_ARG for a missing array, frame or out_base (all checked before a context is looked at) and for an index of another
 *   device than the context's; -LZ4FLEX_E_NO_DEVICE without a device. */
typedef struct lz4flex_frame_index lz4flex_frame_index;
int lz4flex_frame_index_create(lz4flex_ctx *ctx, const void *frame, uint64_t frame_len, int mem_kind, lz4flex_frame_index **out,
                               lz4flex_err_detail *detail /* nullable */);
void lz4flex_frame_index_free(lz4flex_frame_index *x);                      /* NULL is harmless */
uint32_t lz4flex_frame_index_blocks(const lz4flex_frame_index *x);
uint64_t lz4flex_frame_index_content_size(const lz4flex_frame_index *x);    /* decoded bytes of the frame */
uint64_t lz4flex_frame_index_frame_bytes(const lz4flex_frame_index *x);     /* offset behind EndMark (+ content checksum) */
void lz4flex_frame_index_info(const lz4flex_frame_index *x, lz4flex_frame_info *out);
int lz4flex_frame_index_table(const lz4flex_frame_index *x, uint64_t *content_off /* blocks + 1 */, uint64_t *payload_off /* blocks */,
                              uint32_t *len_word /* blocks */);               /* host arrays, any may be NULL */
int lz4flex_frame_read_ranges(lz4flex_ctx *ctx, const lz4flex_frame_index *x, const void *frame, const uint64_t *range_off,
                              const uint64_t *range_len, uint32_t m, void *out_base, const uint64_t *out_off, uint64_t *out_len,
                              int32_t *status, lz4flex_err_detail *detail /* nullable, m entries */, int mem_kind, void *hip_stream);

/* ---- the frame across the GPUs of one node (one process per GPU, an RCCL communicator; BASELINE configs[3]) ----------------
 * FrameEncoder / FrameDecoder for BlockMode::Independent frames whose blocks are spread over `world` ranks: the per-block
 * work of src/frame/compress.rs:261-371 / src/frame/decompress.rs:189-342 runs on every rank for its contiguous block
 * range, ONE exchange step moves the bytes (compress: ncclAllGather of the segment sizes + grouped ncclSend / ncclRecv of the
 * segments to `root`; decompress: the root walks the block headers on its device, broadcasts the table and sends every rank
 * its byte range).  nccl_comm: an ncclComm_t (NULL with world == 1: no RCCL call is made and RCCL is not even loaded).  All
 * data pointers are DEVICE memory; work is enqueued on hip_stream and the calls return after it has completed (they own
 * temporaries).  Linked frames, content checksums / sizes and BlockSize::Auto do not shard: -LZ4FLEX_E_UNSUPPORTED /
 * -LZ4FLEX_E_INVALID_ARG.  Verdicts that depend on the data or on one rank's buffers (a block that failed to compress, a frame
 * that does not parse, a root buffer too small) reach every rank before the exchange they would break: all ranks return the
 * same code and nobody is left waiting.  With more than one rank these entry points have run against a mock communicator
 * (ranks as threads on one device: tests/test_gpu_sharded_native.py; LZ4FLEX_RCCL_LIB names the library that provides the
 * ncclXxx entry points, RCCL by default), never against RCCL on several GPUs (no multi-GPU node was available to this build);
 * lz4_flex_amd/sharded.py is the same exchange over torch.distributed. */
/* bytes a rank's segment can take at most (and the root must be able to receive from it) */
uint64_t lz4flex_frame_segment_bound(uint64_t local_len, const lz4flex_frame_info *info);
/* local[0 .. local_len): this rank's blocks (a multiple of the block size except on the last rank); first_block: the global
 * index of its first block.  On `root`, frame receives header + all segments + EndMark and *frame_len their size (0 elsewhere). */
int lz4flex_frame_compress_sharded(lz4flex_ctx *ctx, void *nccl_comm, int rank, int world, int root, const void *local,
                                   uint64_t local_len, uint64_t first_block, const lz4flex_frame_info *info, void *frame,
                                   uint64_t frame_cap, uint64_t *frame_len, void *hip_stream);
/* frame / frame_bytes: needed on `root` only.  Every rank decodes blocks [*first_block, *first_block + *n_blocks) into out (block i of
 * the range at i * block size), *out_len bytes; info_out (nullable) receives the frame's block size and checksum flag. */
int lz4flex_frame_decompress_sharded(lz4flex_ctx *ctx, void *nccl_comm, int rank, int world, int root, const void *frame,
                                     uint64_t frame_bytes, void *out, uint64_t out_cap, uint64_t *out_len, uint64_t *first_block,
                                     uint64_t *n_blocks, lz4flex_frame_info *info_out, lz4flex_err_detail *detail, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* LZ4FLEX_AMD_H */
