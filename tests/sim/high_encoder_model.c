// high_encoder_model.c -- the scalar DEFINITION of compress_mode 2 ("high", lz4_flex_amd/csrc/lz4_compress_high.hip): the kernel gives
// these bytes for every block and every depth.  Test infrastructure (tests/hc_model.py builds it on demand).
//
// A block in[0, n) and a depth K (1 .. 256):
//   chunks      positions below 65 536 are chunk 0 = [0, 65 536), base 0; a later position p lies in the chunk
//               [p & ~32767, + 32 768) with base = chunk start - 32 768: a chunk sees at most 64 KiB, an offset is at most 65 535.
//   candidates  every position p <= n - 12 has the hash (load32(p) * 2654435761u) >> 17; the candidates of p are the earlier positions
//               q >= base(p) with p's hash, nearest first, at most K of them (a hash collision counts as one of the K).
//   best[p]     a candidate matches if its first 4 bytes equal p's; its length is counted up to lim = min(chunk end, n - 5) - p;
//               best[p] is the longest match of at least 4 bytes, the nearest one of equal lengths; none: length 0.
//   parse       a function of best[] alone: from p = 0; best[p].len < 4: p is a literal; p + 1 in p's chunk and
//               best[p + 1].len > best[p].len: p is a literal (one-step lazy); otherwise the sequence (literals since the anchor,
//               offset, len) and p += len.  The trailing literals close the block.
// Matches end at their chunk's end at the latest, so every chunk is parsed from its own first position.
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define LZ4H_HASH_BITS 15u
#define LZ4H_CHUNK0 65536u
#define LZ4H_CHUNK 32768u

typedef struct { uint32_t len, off; } lz4h_best;

static uint32_t load32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
static uint64_t load64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }
static uint32_t hash_of(const uint8_t* p) { return (load32(p) * 2654435761u) >> (32u - LZ4H_HASH_BITS); }

static uint8_t* put_len(uint8_t* o, uint32_t r) {
    while (r >= 255u) { *o++ = 255u; r -= 255u; }
    *o++ = (uint8_t)r;
    return o;
}

// best[] of the chunk [cs, ce) (positions relative to cs), written for every position of the chunk that lies in the block
static void chunk_best(const uint8_t* in, uint32_t n, uint32_t cs, uint32_t ce, uint32_t depth, lz4h_best* best, int32_t* head, int32_t* prev) {
    const uint32_t base = cs == 0u ? 0u : cs - LZ4H_CHUNK;
    const uint32_t end = ce < n ? ce : n;                       // the chunk's positions that exist
    const uint32_t mend = ce < n - 5u ? ce : n - 5u;            // where a match of this chunk ends at the latest
    for (uint32_t h = 0; h < (1u << LZ4H_HASH_BITS); ++h) head[h] = -1;
    for (uint32_t p = base; p < end; ++p) {
        lz4h_best b = {0u, 0u};
        if (p + 12u <= n) {
            const uint32_t h = hash_of(in + p);
            if (p >= cs) {
                const uint32_t lim = mend - p, v = load32(in + p);
                int32_t q = head[h];
                for (uint32_t k = 0; k < depth && q >= 0; ++k, q = prev[(uint32_t)q - base]) {
                    if (load32(in + q) != v) continue;
                    uint32_t l = 4u;
                    while (l + 8u <= lim && load64(in + (uint32_t)q + l) == load64(in + p + l)) l += 8u;
                    while (l < lim && in[(uint32_t)q + l] == in[p + l]) ++l;
                    if (l > lim) l = lim;                       // (the chunk ends less than 4 bytes behind p)
                    if (l >= 4u && l > b.len) { b.len = l; b.off = p - (uint32_t)q; }
                    if (b.len == lim) break;                    // nothing is longer, and an equal one does not replace it
                }
            }
            prev[p - base] = head[h];
            head[h] = (int32_t)p;
        }
        if (p >= cs) best[p - cs] = b;
    }
}

// out holds 20 + n * 110 / 100 bytes; returns the block's length
size_t lz4h_compress(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t depth) {
    uint8_t* o = out;
    uint32_t anchor = 0;
    if (n >= 12u) {
        lz4h_best* best = (lz4h_best*)malloc(sizeof(lz4h_best) * (LZ4H_CHUNK0 + 1u));
        int32_t* head = (int32_t*)malloc(sizeof(int32_t) << LZ4H_HASH_BITS);
        int32_t* prev = (int32_t*)malloc(sizeof(int32_t) * LZ4H_CHUNK0);
        for (uint32_t cs = 0; cs + 12u <= n;) {
            const uint32_t ce = cs == 0u ? LZ4H_CHUNK0 : (cs + LZ4H_CHUNK < cs ? 0xFFFFFFFFu : cs + LZ4H_CHUNK);
            const uint32_t end = ce < n ? ce : n;
            chunk_best(in, n, cs, ce, depth, best, head, prev);
            best[end - cs].len = 0u;                            // (read as best[p + 1] where the block ends inside the chunk)
            for (uint32_t p = cs; p < end;) {
                const lz4h_best b = best[p - cs];
                if (b.len < 4u || (p + 1u < ce && best[p + 1u - cs].len > b.len)) { ++p; continue; }
                const uint32_t lit = p - anchor, ml = b.len - 4u;
                *o++ = (uint8_t)(((lit < 15u ? lit : 15u) << 4) | (ml < 15u ? ml : 15u));
                if (lit >= 15u) o = put_len(o, lit - 15u);
                memcpy(o, in + anchor, lit); o += lit;
                *o++ = (uint8_t)b.off; *o++ = (uint8_t)(b.off >> 8);
                if (ml >= 15u) o = put_len(o, ml - 15u);
                p += b.len;
                anchor = p;
            }
            if (ce >= n) break;
            cs = ce;
        }
        free(best); free(head); free(prev);
    }
    const uint32_t lit = n - anchor;
    *o++ = (uint8_t)((lit < 15u ? lit : 15u) << 4);
    if (lit >= 15u) o = put_len(o, lit - 15u);
    memcpy(o, in + anchor, lit); o += lit;
    return (size_t)(o - out);
}
