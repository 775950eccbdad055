// high_optimal_model.c -- the scalar DEFINITION of compress_mode 2 ("high") under "compress_parse" 1, the optimal parse
// (lz4_flex_amd/csrc/lz4_compress_high.hip, step 3 1/2): the kernel gives these bytes for every (block, dictionary, depth).  Test
// infrastructure (tests/hc_optimal_model.py builds it on demand).
//
// Chunks, candidates and best[] are high_encoder_model.c's, with a dictionary or a history high_dict_model.c's: their chunk_best /
// chunk_best_dict are called as they stand.  parse 0 is their one-step lazy parse (the same bytes); parse 1 replaces best[].len by len'[]:
// a price-based backward pass over every chunk, in segments of S = 2 048 positions that know nothing of each other.  For a chunk with cn
// positions (j relative to its start; ext(v) = the length bytes behind a token nibble):
//   for j = cn - 1 down to 0:
//       se = min((j / S + 1) * S, cn)                  the end of j's segment; CO(x) = x >= se ? 0 : cost[x]
//       L = best[j].len; c = infinity; pick = 0
//       if L >= 4:  Lp = min(L, se - j)                the part of the match that is priced
//                   c = 3 + ext(Lp < 4 ? 0 : Lp - 4) + CO(j + L); pick = L
//                   for l = min(L - 1, 35, se - j) down to 4: v = 3 + ext(l - 4) + CO(j + l); if v < c: c = v, pick = l
//       if 1 + CO(j + 1) < c: c = 1 + CO(j + 1), pick = 0
//       cost[j] = c; len'[j] = pick
// and the walk takes len'[j] >= 4 as a match of that length at best[j].off, anything else as a literal; there is no lazy test.  Ties go to
// the full length, then to the longer short length, the literal last.  A literal run's own length bytes are not priced.
#include "high_dict_model.c"

#define LZ4HO_SEG 2048u
#define LZ4HO_SHORT_MAX 35u

static uint32_t ext_of(uint32_t v) { return v < 15u ? 0u : (v - 15u) / 255u + 1u; }

// len'[0, cn) of a chunk from its best[0, cn); cost: cn + 1 words of scratch
static void optimal_lengths(const lz4h_best* best, uint32_t cn, uint32_t* pick, uint32_t* cost) {
    for (uint32_t j = cn; j-- > 0u;) {
        const uint32_t se0 = (j / LZ4HO_SEG + 1u) * LZ4HO_SEG, se = se0 < cn ? se0 : cn;
#define CO(x) ((x) >= se ? 0u : cost[x])
        const uint32_t L = best[j].len, room = se - j;
        uint32_t c = 0xFFFFFFFFu, pk = 0u;
        if (L >= 4u) {
            const uint32_t lp = L < room ? L : room;
            c = 3u + ext_of(lp < 4u ? 0u : lp - 4u) + CO(j + L);
            pk = L;
            uint32_t l = L - 1u;
            if (l > LZ4HO_SHORT_MAX) l = LZ4HO_SHORT_MAX;
            if (l > room) l = room;
            for (; l >= 4u; --l) {
                const uint32_t v = 3u + ext_of(l - 4u) + CO(j + l);
                if (v < c) { c = v; pk = l; }
            }
        }
        if (1u + CO(j + 1u) < c) { c = 1u + CO(j + 1u); pk = 0u; }
#undef CO
        cost[j] = c;
        pick[j] = pk;
    }
}

// out holds 20 + n * 110 / 100 bytes; returns the block's length.  dict_len < 4: no dictionary.  t_len / t_off / t_pick (nullable, n words
// each): best[].len, best[].off and the length the walk reads (parse 0: best[].len) of every position of the block.
size_t lz4ho_compress_trace(const uint8_t* in, uint32_t n, const uint8_t* dict, uint32_t dict_len, uint8_t* out, uint32_t depth, uint32_t parse,
                            uint32_t* t_len, uint32_t* t_off, uint32_t* t_pick) {
    const uint32_t h = dict_len < 4u ? 0u : (dict_len < LZ4H_CHUNK ? dict_len : LZ4H_CHUNK);
    uint8_t* o = out;
    uint32_t anchor = 0;
    if (t_len) for (uint32_t i = 0; i < n; ++i) t_len[i] = t_off[i] = t_pick[i] = 0u;
    if (n >= 12u) {
        uint8_t* s = (uint8_t*)malloc((size_t)h + n);
        lz4h_best* best = (lz4h_best*)malloc(sizeof(lz4h_best) * (LZ4H_CHUNK0 + 1u));
        int32_t* head = (int32_t*)malloc(sizeof(int32_t) << LZ4H_HASH_BITS);
        int32_t* prev = (int32_t*)malloc(sizeof(int32_t) * LZ4H_CHUNK0);
        uint32_t* pick = (uint32_t*)malloc(sizeof(uint32_t) * (LZ4H_CHUNK0 + 1u));
        uint32_t* cost = (uint32_t*)malloc(sizeof(uint32_t) * (LZ4H_CHUNK0 + 1u));
        if (h) memcpy(s, dict + (dict_len - h), h);
        memcpy(s + h, in, n);
        for (uint32_t cs = 0; cs + 12u <= n;) {
            const uint32_t size = (cs == 0u && h == 0u) ? LZ4H_CHUNK0 : LZ4H_CHUNK;
            const uint32_t ce = cs + size < cs ? 0xFFFFFFFFu : cs + size;
            const uint32_t end = ce < n ? ce : n, cn = end - cs;
            if (h) chunk_best_dict(s, h, n, cs, ce, depth, best, head, prev);
            else chunk_best(in, n, cs, ce, depth, best, head, prev);
            best[cn].len = 0u;
            if (parse) optimal_lengths(best, cn, pick, cost);
            else for (uint32_t j = 0; j < cn; ++j) pick[j] = best[j].len;
            if (t_len) for (uint32_t j = 0; j < cn; ++j) { t_len[cs + j] = best[j].len; t_off[cs + j] = best[j].off; t_pick[cs + j] = pick[j]; }
            for (uint32_t p = cs; p < end;) {
                const uint32_t len = pick[p - cs], off = best[p - cs].off;
                if (len < 4u || (!parse && p + 1u < ce && best[p + 1u - cs].len > len)) { ++p; continue; }
                const uint32_t lit = p - anchor, ml = len - 4u;
                *o++ = (uint8_t)(((lit < 15u ? lit : 15u) << 4) | (ml < 15u ? ml : 15u));
                if (lit >= 15u) o = put_len(o, lit - 15u);
                memcpy(o, in + anchor, lit); o += lit;
                *o++ = (uint8_t)off; *o++ = (uint8_t)(off >> 8);
                if (ml >= 15u) o = put_len(o, ml - 15u);
                p += len;
                anchor = p;
            }
            if (ce >= n) break;
            cs = ce;
        }
        free(s); free(best); free(head); free(prev); free(pick); free(cost);
    }
    const uint32_t lit = n - anchor;
    *o++ = (uint8_t)((lit < 15u ? lit : 15u) << 4);
    if (lit >= 15u) o = put_len(o, lit - 15u);
    memcpy(o, in + anchor, lit); o += lit;
    return (size_t)(o - out);
}

size_t lz4ho_compress(const uint8_t* in, uint32_t n, const uint8_t* dict, uint32_t dict_len, uint8_t* out, uint32_t depth, uint32_t parse) {
    return lz4ho_compress_trace(in, n, dict, dict_len, out, depth, parse, NULL, NULL, NULL);
}
