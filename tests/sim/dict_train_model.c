// dict_train_model.c -- the scalar definition of lz4flex_dict_train (lz4_flex_amd/csrc/lz4_dict_train.hip): the kernels equal it byte
// for byte.  A dictionary of at most `cap` bytes is a concatenation of segments of at most k bytes cut from the samples, chosen by a
// fastCover-style rule in which every step is an integer computation with a fixed result:
//   candidates   the positions p of a sample with 8 bytes left (p + 8 <= len), numbered globally in batch order; total = their number
//   hash(p)      (LE64(sample[p .. p + 8)) * 0x9E3779B185EBCA87) >> 44: 20 bits
//   freq[h]      how many candidates of the whole batch have hash h
//   first(p)     0 if one of the k - 1 candidates in front of p IN ITS SAMPLE has p's hash, else 1
//   w(p)         first(p) ? min(freq[hash(p)], 2^20 - 1) : 0, with the table as it stands when it is read
//   score(s)     the sum of w(p) over p in [s, min(s + k - 7, c)), c = the sample's candidates: the 8-byte windows inside the k bytes at s
//   regions      nseg = ceil(cap / k), E = max(1, min(nseg, total / (4 k))), R = ceil(total / E): region r = global numbers [r R, (r + 1) R)
//   step t       (t = 0 .. 2 nseg - 1; ends when no capacity is left or E steps in a row chose nothing) the start of region t mod E with
//                the largest score, the lowest number among equals; score 0 chooses nothing; else the segment sample[s .. s + min(k,
//                len - s)) is chosen, clipped to the capacity that is left, and the counters of its windows are set to 0
//   output       the chosen segments in REVERSE order of choice: the best material at the tail, which is what the encoders look at.
// Plain and quadratic where that is simplest: it is the definition.  Test infrastructure.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define DTM_F 20
#define DTM_WMAX ((1u << 20) - 1u)
#define DTM_E_UNSUPPORTED 68

static uint32_t hash8(const uint8_t* p) {
    uint64_t v = 0;
    for (int b = 0; b < 8; b++) v |= (uint64_t)p[b] << (8 * b);
    return (uint32_t)((v * 0x9E3779B185EBCA87ull) >> (64 - DTM_F));
}

static uint32_t candidates(uint32_t len) { return len >= 8u ? len - 7u : 0u; }

// picks (nullable): 3 words per chosen segment in the order of choice -- sample, start, bytes taken; *n_picks their number.
// Returns 0, or -1 when memory ran out.
int dtm_train(const uint8_t* base, const uint64_t* off, const uint32_t* len, uint32_t n, uint8_t* out, uint32_t cap, uint32_t k,
              uint32_t* dict_len, int32_t* status, uint32_t* picks, uint32_t* n_picks) {
    *dict_len = 0; *status = 0;
    if (n_picks) *n_picks = 0;
    if (k == 0) k = 512;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) total += candidates(len[i]);
    if (total >> 32) { *status = DTM_E_UNSUPPORTED; return 0; }
    if (total == 0 || cap == 0) return 0;

    uint32_t* freq = calloc(1u << DTM_F, 4);
    uint32_t* hash = malloc(total * 4);            // by global number
    uint8_t* first = malloc(total);
    uint64_t* cstart = malloc(((uint64_t)n + 1) * 8);
    uint8_t* stage = malloc(cap);                  // filled from the back
    uint64_t* prefix = NULL;
    if (!freq || !hash || !first || !cstart || !stage) { free(freq); free(hash); free(first); free(cstart); free(stage); return -1; }

    uint64_t g = 0;
    for (uint32_t i = 0; i < n; i++) {
        cstart[i] = g;
        const uint32_t c = candidates(len[i]);
        for (uint32_t p = 0; p < c; p++) {
            const uint32_t h = hash8(base + off[i] + p);
            hash[g + p] = h;
            freq[h]++;
            first[g + p] = 1;
            for (uint32_t q = p >= k - 1 ? p - (k - 1) : 0; q < p; q++)      // p - k < q < p
                if (hash[g + q] == h) { first[g + p] = 0; break; }
        }
        g += c;
    }
    cstart[n] = g;

    const uint32_t nseg = (cap + k - 1) / k;
    uint64_t E = total / (4ull * k);
    if (E > nseg) E = nseg;
    if (E < 1) E = 1;
    const uint64_t R = (total + E - 1) / E;
    uint32_t remaining = cap, zero_run = 0, chosen = 0;
    int rc = 0;

    for (uint32_t t = 0; t < 2 * nseg && remaining != 0 && zero_run < E; t++) {
        const uint64_t lo = (t % E) * R, hi = lo + R < total ? lo + R : total;
        uint64_t best_score = 0, best_g = 0;
        uint32_t best_i = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t c = cstart[i + 1] - cstart[i];
            if (c == 0 || cstart[i + 1] <= lo || cstart[i] >= hi) continue;
            // prefix[p] = w(0) + ... + w(p - 1) over the sample
            uint64_t* bigger = realloc(prefix, (c + 1) * 8);
            if (!bigger) { rc = -1; goto done; }
            prefix = bigger;
            prefix[0] = 0;
            for (uint64_t p = 0; p < c; p++) {
                const uint32_t f = freq[hash[cstart[i] + p]];
                prefix[p + 1] = prefix[p] + (first[cstart[i] + p] ? (f < DTM_WMAX ? f : DTM_WMAX) : 0u);
            }
            const uint64_t s0 = lo > cstart[i] ? lo - cstart[i] : 0, s1 = (hi < cstart[i + 1] ? hi : cstart[i + 1]) - cstart[i];
            for (uint64_t s = s0; s < s1; s++) {
                const uint64_t e = s + k - 7 < c ? s + k - 7 : c;
                const uint64_t score = prefix[e] - prefix[s];
                if (score > best_score) { best_score = score; best_g = cstart[i] + s; best_i = i; }      // (ascending numbers: the first of equals stays)
            }
        }
        if (best_score == 0) { zero_run++; continue; }
        zero_run = 0;
        const uint32_t s = (uint32_t)(best_g - cstart[best_i]), c = candidates(len[best_i]);
        const uint32_t L = len[best_i] - s < k ? len[best_i] - s : k;
        const uint32_t take = L < remaining ? L : remaining;
        memcpy(stage + remaining - take, base + off[best_i] + s, take);
        for (uint32_t p = s; p < c && p < s + k - 7; p++) freq[hash[best_g - s + p]] = 0;
        remaining -= take;
        if (picks) { picks[3 * chosen] = best_i; picks[3 * chosen + 1] = s; picks[3 * chosen + 2] = take; }
        chosen++;
    }
done:
    if (rc == 0) {
        *dict_len = cap - remaining;
        memcpy(out, stage + remaining, cap - remaining);
        if (n_picks) *n_picks = chosen;
    }
    free(freq); free(hash); free(first); free(cstart); free(stage); free(prefix);
    return rc;
}
