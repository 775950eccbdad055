// high_dict_model.c -- the scalar DEFINITION of compress_mode 2 ("high") against an external dictionary ("compress_high_dict" 1,
// lz4_flex_amd/csrc/lz4_compress_high.hip, the dictionary form): the kernel gives these bytes for every (block, dictionary, depth).
// Test infrastructure (tests/hc_dict_model.py builds it on demand).  Candidates, best[] and the parse are high_encoder_model.c's; what a
// dictionary changes:
//   history     H = dict_len < 4 ? 0 : min(dict_len, 32 768).  H == 0: lz4h_compress's bytes.  Otherwise the stream is
//               S = dict[dict_len - H ..] ++ in, block position p is S position H + p.
//   chunks      every chunk is 32 KiB: chunk c = block positions [c * 32 768, + 32 768); its base lies 32 768 positions earlier in S and
//               not below S position 0 -- chunk 0 sees the dictionary's tail and itself, every later chunk the block alone.
//   hashes      block positions p <= n - 12 and tail positions q with q + 4 <= H; the three tail positions whose 4 bytes straddle the
//               dictionary's end have none and are never candidates (the dictionary's order is a function of the dictionary alone).
//   lengths     counted over S (a match may start in the dictionary and run on into the block) up to lim = min(chunk end, n - 5) - p.
#include "high_encoder_model.c"

// best[] of the chunk [cs, ce) of the block (positions relative to cs); s = S, h = H
static void chunk_best_dict(const uint8_t* s, uint32_t h, uint32_t n, uint32_t cs, uint32_t ce, uint32_t depth, lz4h_best* best, int32_t* head,
                            int32_t* prev) {
    const uint32_t base = h + cs < LZ4H_CHUNK ? 0u : h + cs - LZ4H_CHUNK;      // S positions from here on
    const uint32_t end = ce < n ? ce : n;
    const uint32_t mend = ce < n - 5u ? ce : n - 5u;
    for (uint32_t x = 0; x < (1u << LZ4H_HASH_BITS); ++x) head[x] = -1;
    for (uint32_t sp = base; sp < h + end; ++sp) {
        lz4h_best b = {0u, 0u};
        if (sp < h ? sp + 4u <= h : sp - h + 12u <= n) {
            const uint32_t hv = hash_of(s + sp);
            if (sp >= h + cs) {
                const uint32_t lim = mend - (sp - h), v = load32(s + sp);
                int32_t q = head[hv];
                for (uint32_t k = 0; k < depth && q >= 0; ++k, q = prev[(uint32_t)q - base]) {
                    if (load32(s + q) != v) continue;
                    uint32_t l = 4u;
                    while (l + 8u <= lim && load64(s + (uint32_t)q + l) == load64(s + sp + l)) l += 8u;
                    while (l < lim && s[(uint32_t)q + l] == s[sp + l]) ++l;
                    if (l > lim) l = lim;
                    if (l >= 4u && l > b.len) { b.len = l; b.off = sp - (uint32_t)q; }
                    if (b.len == lim) break;
                }
            }
            prev[sp - base] = head[hv];
            head[hv] = (int32_t)sp;
        }
        if (sp >= h + cs) best[sp - h - cs] = b;
    }
}

// out holds 20 + n * 110 / 100 bytes; returns the block's length
size_t lz4h_compress_dict(const uint8_t* in, uint32_t n, const uint8_t* dict, uint32_t dict_len, uint8_t* out, uint32_t depth) {
    const uint32_t h = dict_len < 4u ? 0u : (dict_len < LZ4H_CHUNK ? dict_len : LZ4H_CHUNK);
    if (h == 0u) return lz4h_compress(in, n, out, depth);
    uint8_t* o = out;
    uint32_t anchor = 0;
    if (n >= 12u) {
        uint8_t* s = (uint8_t*)malloc((size_t)h + n);
        lz4h_best* best = (lz4h_best*)malloc(sizeof(lz4h_best) * (LZ4H_CHUNK + 1u));
        int32_t* head = (int32_t*)malloc(sizeof(int32_t) << LZ4H_HASH_BITS);
        int32_t* prev = (int32_t*)malloc(sizeof(int32_t) * 2u * LZ4H_CHUNK);
        memcpy(s, dict + (dict_len - h), h);
        memcpy(s + h, in, n);
        for (uint32_t cs = 0; cs + 12u <= n;) {
            const uint32_t ce = cs + LZ4H_CHUNK < cs ? 0xFFFFFFFFu : cs + LZ4H_CHUNK;
            const uint32_t end = ce < n ? ce : n;
            chunk_best_dict(s, h, n, cs, ce, depth, best, head, prev);
            best[end - cs].len = 0u;
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
        free(s); free(best); free(head); free(prev);
    }
    const uint32_t lit = n - anchor;
    *o++ = (uint8_t)((lit < 15u ? lit : 15u) << 4);
    if (lit >= 15u) o = put_len(o, lit - 15u);
    memcpy(o, in + anchor, lit); o += lit;
    return (size_t)(o - out);
}
