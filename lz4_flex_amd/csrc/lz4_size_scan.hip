// lz4_size_scan.hip -- batched decompressed-size query for raw LZ4 blocks, gfx950 (lz4flex_decompressed_size_batch).
//
// For every block: the number of bytes lz4_flex::block::decompress_into (src/block/decompress.rs:201-449) would produce with an
// unbounded sink and `history` bytes in front of the block's output, or the DecompressError it would return.  Nothing is decoded: only
// the token chain is followed, the lengths summed, and the checks that need a position (offset <= position, :399-401) made.
//
// Two passes, the scheme of the decoders (lz4_decompress_seq.hip + lz4_decompress.hip):
//   * PARALLEL (lz4_size_scan_kernel): one block per WAVEFRONT, the shape of the sequence decoder without its copies and window.  The
//     compressed stream is staged in LDS in tiles of 3 840 bytes (zeros behind the block); 64 lanes walk 64 parts of a tile from
//     assumed entries and the true chain is resolved from the tile's entry (the WALK both kernels share: lz4_seq_walk.h), the set bits
//     of the live parts are the tile's token list.  Then CHUNKS of 64 consecutive sequences, lane =
//     sequence: token, literal length, offset and match length from the staged tile, a DPP prefix sum of literal + match lengths places
//     all 64, and every reference check is one ballot (literals past the input :346-348, an offset missing :373-375, offset zero
//     :168-173, offset behind the output :399-401, a match that ends the block :439-443).  A sequence whose lengths do not fit a lane
//     (a literal run of more than LITMAX bytes, any length with a 255 byte) is measured by the whole wavefront from memory, 64 length
//     bytes per load.  A block with anything suspicious -- every error, a position beyond POS_LIMIT, a walk that does not settle -- is
//     marked REDO and left alone.
//   * SERIAL (lz4_size_serial_kernel): one LANE per marked block, the reference's loop restated line by line with 64-bit positions:
//     the error variant comes from code in the reference's check order.  "size_scan_serial" 1 sends every block there (tests).
// LDS per wavefront: token list 2 560 + tile 4 080 = 6 640 bytes.  Nothing is written but out_size[b] and status[b].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4_device.h"
#include "lz4_seq_walk.h"

namespace lz4flex_dev {
namespace ss {

using namespace sw;      // the walk, its geometry and the lane / LDS helpers

constexpr uint32_t LITMAX = 192u;            // literal run whose offset and match length a lane reads from the staged tile
constexpr uint32_t LDS_BYTES = LDS_TILE + TILE_LDS;
// a token at PT - 1: literals from PT + 1, LITMAX of them, then the offset and a match length byte, read as two aligned dwords
static_assert(((PT + 1u + LITMAX) & ~3u) + 8u <= PT + TMARGIN, "a lane's offset and match length byte lie inside the staged bytes");

// ---- measuring --------------------------------------------------------------------------------------------------------------------
// (a length run by the whole wavefront: run_len, lz4_seq_walk.h)
// (one sequence of any shape by the whole wavefront: wave_seq, lz4_seq_walk.h)
// The sequences [0, n_tile) of the tile's token list, 64 at a time.  op advances; false: the block goes to the serial pass.
__device__ __forceinline__ bool run_chunks(const g_u8* in, uint32_t ilen, uint32_t lane, uint32_t hist, uint32_t t0, uint32_t n_tile,
                                           uint32_t& op, bool& done) {
    const uint32_t ilr = ilen - t0;
    uint32_t sidx = 0u;
    while (sidx < n_tile) {
        sidx = uni(sidx); op = uni(op);
        const uint32_t nrem = n_tile - sidx;
        // token, lengths, offset (decompress.rs:249-258, 334-391)
        const Token t = decode_token<LITMAX>(sidx + (lane < nrem ? lane : nrem - 1u), ilr);
        const uint32_t tpr = t.tpr, lit = t.lit, off = t.off, mlx = t.mlx;
        const uint64_t lastm = t.lastm;
        uint64_t errm, bigm;
        chunk_masks(t, ilr, errm, bigm);
        uint32_t nact = nrem < 64u ? nrem : 64u;
        {
            const uint64_t bm = bigm & low_mask(nact);
            if (bm != 0ull) nact = ctz64(bm);
        }
        if (nact == 0u) {                                      // the sequence alone, by the whole wavefront
            const uint32_t tp0 = rdlane(tpr, 0u);
            uint32_t sl, sm;
            if (!wave_seq(in, ilen, lane, hist, t0 + tp0, op, sl, sm, done)) return false;
            sidx += 1u;
            if (done) return sidx == n_tile;
            continue;
        }
        const uint64_t am = low_mask(nact);
        if ((errm & am) != 0ull) return false;
        if ((lastm & low_mask(nact - 1u)) != 0ull) return false;   // (a token behind the block's last sequence: not a real chain)
        const uint32_t ml = lanes(lastm) ? 0u : mlx;
        const uint32_t u = lanes(am) ? lit + ml : 0u;
        const uint32_t incl = wave_incl_add(u);
        const uint32_t T = rdlane(incl, nact - 1u);
        if ((uint64_t)op + T > POS_LIMIT) return false;
        const uint32_t dm = op + incl - u + lit;               // output position of the match
        if ((ballot((uint64_t)off > (uint64_t)dm + hist) & ~lastm & am) != 0ull) return false;   // OffsetOutOfBounds (:399-401)
        op += T;
        sidx += nact;
        if (((lastm >> (nact - 1u)) & 1ull) != 0ull) { done = true; return sidx == n_tile; }
    }
    return true;
}

__global__ void __launch_bounds__(64) lz4_size_scan_kernel(const uint8_t* in_base, const uint64_t* in_off, const uint32_t* in_len,
                                                          const uint32_t* history, uint32_t n, uint64_t* out_size, int32_t* status,
                                                          int32_t redo_code) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ss_lds[];
    const uint32_t lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    if (b >= n) return;
    // (every LDS access below goes by byte address from 0: the dynamic segment is the kernel's only LDS)
    if ((uint32_t)(uintptr_t)(lds_u8*)ss_lds != 0u) { if (lane == 0u) { status[b] = redo_code; out_size[b] = 0u; } return; }
    const g_u8* in = (const g_u8*)(in_base + in_off[b]);
    const uint32_t ilen = in_len[b];
    const uint32_t hist = history != nullptr ? uni(history[b]) : 0u;
    bool ok = ilen != 0u && ilen <= POS_LIMIT, done = false;   // (the empty block, decompress.rs:207-209: the serial pass reports it)
    uint32_t op = 0u, entry = 0u;
    if (lane < 4u) lds_wr4(LDS_TILE + 4u * lane, 0u);         // the bytes in front of the first tile
    for (;;) {
        entry = uni(entry); op = uni(op);
        if (uni((ok && !done) ? 1u : 0u) == 0u) break;
        const uint32_t t0 = entry & ~15u;
        stage_tile(in, ilen, t0, lane);
        const uint32_t ilr = ilen - t0;
        const uint32_t entry_r = entry - t0;
        Part s;
        first_walks(in, ilen, t0, lane, entry_r, s);
        uint32_t my_entry, rounds;
        const uint32_t tile_exit = settle_chain(in, ilen, t0, lane, entry_r, s, my_entry, rounds);
        if (tile_exit == X_ERR) { ok = false; break; }
        const uint32_t n_tile = write_token_list(lane, my_entry, s);
        if (n_tile > POSCAP || n_tile == 0u) { ok = false; break; }
        // ---- the sequences -----------------------------------------------------------------------------------------------------------
        bool tdone = false;
        if (!run_chunks(in, ilen, lane, hist, t0, n_tile, op, tdone)) { ok = false; break; }
        if (tdone) { done = true; break; }
        if (tile_exit >= ilr) { ok = false; break; }        // the chain ran out without a last sequence
        entry = t0 + tile_exit;
    }
    if (lane == 0u) {
        if (ok && done) { status[b] = 0; out_size[b] = op; }
        else { status[b] = redo_code; out_size[b] = 0u; }
    }
}

// ---- the serial pass: decompress.rs:201-449 for one block per lane, lengths only, 64-bit positions -----------------------------------
__device__ int32_t measure_block(const uint8_t* in, uint64_t ilen, uint64_t hist, uint64_t& size) {
    if (ilen == 0u) return LZ4FLEX_DEV_E_EXPECTED_ANOTHER_BYTE;           // :207-209
    uint64_t ip = 0u, op = 0u;
    for (;;) {
        const uint32_t token = in[ip++];                                  // :249-250
        uint64_t lit = token >> 4;                                        // :334
        if (lit != 0u) {
            if (lit == 15u) {                                             // :336-340
                const int32_t e = read_integer(in, ilen, ip, lit);
                if (e) return e;
            }
            if (lit > ilen - ip) return LZ4FLEX_DEV_E_LITERAL_OUT_OF_BOUNDS;      // :346-348
            op += lit;
            ip += lit;
        }
        if (ip >= ilen) break;                                            // :366-368
        if (ilen - ip < 2u) return LZ4FLEX_DEV_E_EXPECTED_ANOTHER_BYTE;  // :373-375
        const uint64_t offset = (uint64_t)in[ip] | ((uint64_t)in[ip + 1u] << 8);
        ip += 2u;
        if (offset == 0u) return LZ4FLEX_DEV_E_OFFSET_ZERO;               // :168-173
        uint64_t ml = 4u + (token & 0xFu);                                // :386-391
        if (ml == 19u) {
            const int32_t e = read_integer(in, ilen, ip, ml);
            if (e) return e;
        }
        if (offset > op + hist) return LZ4FLEX_DEV_E_OFFSET_OUT_OF_BOUNDS;        // :399-401
        op += ml;
        if (ip >= ilen) return LZ4FLEX_DEV_E_EXPECTED_ANOTHER_BYTE;       // :439-443
    }
    size = op;
    return 0;
}

__global__ void __launch_bounds__(256) lz4_size_serial_kernel(const uint8_t* in_base, const uint64_t* in_off, const uint32_t* in_len,
                                                             const uint32_t* history, uint32_t n, uint64_t* out_size, int32_t* status,
                                                             int32_t only_status) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= n) return;
    if (only_status != 0 && status[b] != only_status) return;
    uint64_t size = 0u;
    const int32_t st = measure_block(in_base + in_off[b], in_len[b], history != nullptr ? history[b] : 0u, size);
    status[b] = st;
    out_size[b] = st == 0 ? size : 0u;
}

}  // namespace ss

hipError_t launch_size_scan(const uint8_t* in_base, const uint64_t* in_off, const uint32_t* in_len, const uint32_t* history, uint32_t n,
                            uint64_t* out_size, int32_t* status, int serial_only, hipStream_t s) {
    if (n == 0u) return hipSuccess;
    const int32_t redo = SIZE_SCAN_REDO;
    if (!serial_only) {
        hipLaunchKernelGGL(ss::lz4_size_scan_kernel, dim3(n), dim3(64), ss::LDS_BYTES, s, in_base, in_off, in_len, history, n, out_size,
                           status, redo);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(ss::lz4_size_serial_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, in_base, in_off, in_len, history, n, out_size,
                       status, serial_only ? 0 : redo);
    return hipGetLastError();
}

}  // namespace lz4flex_dev
