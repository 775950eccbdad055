// frame_range_shim.cpp -- lz4_flex_amd/csrc/frame_range.h behind a C interface, for tests/test_frame_range_plan.py (a CPU test: the
// header is host-only integer arithmetic).  FRAME_RANGE_SHIM_MAIN: the same walk as a stand-alone program (its own main), for a
// sanitizer build outside Python.
#include <cstdint>
#include <vector>

#include "../../lz4_flex_amd/csrc/frame_range.h"

using namespace lz4flex_range;

extern "C" {

uint64_t fr_rec_bytes() { return sizeof(RangeRec); }
uint64_t fr_head_align() { return HEAD_ALIGN; }
uint64_t fr_pass_slots_max() { return PASS_SLOTS_MAX; }

// out[0 .. 5): clipped length, b0, nb, head, head_bytes
void fr_locate(const uint64_t* content_off, const uint32_t* len_word, uint32_t n, uint64_t off, uint64_t len, uint64_t* out) {
    RangeRec r{};
    locate(content_off, len_word, n, off, len, &r);
    out[0] = r.len; out[1] = r.b0; out[2] = r.nb; out[3] = r.head; out[4] = r.head_bytes;
}

// every range located, then cut into passes; cost: nullable (then a range costs its head's scratch slot).  per[4 r ..]: pass, slot,
// head_off, the pass's slots; returns the number of passes
uint32_t fr_plan(const uint64_t* content_off, const uint32_t* len_word, uint32_t n, const uint64_t* off, const uint64_t* len, uint32_t m,
                 const uint64_t* cost, uint64_t pass_bytes, uint64_t* per) {
    std::vector<RangeRec> recs(m);
    std::vector<uint64_t> c(m);
    for (uint32_t r = 0; r < m; r++) {
        recs[r] = RangeRec{};
        locate(content_off, len_word, n, off[r], len[r], &recs[r]);
        c[r] = cost ? cost[r] : head_slot_bytes(recs[r]);
    }
    uint32_t passes = 0;
    for (uint32_t first = 0; first < m; passes++) {
        uint64_t slots = 0, heads = 0;
        const uint32_t cnt = cut_pass(recs.data(), c.data(), first, m, pass_bytes, &slots, &heads);
        for (uint32_t r = first; r < first + cnt; r++) {
            per[4 * r] = passes; per[4 * r + 1] = recs[r].slot; per[4 * r + 2] = recs[r].head_off; per[4 * r + 3] = slots;
        }
        first += cnt;
    }
    return passes;
}

}  // extern "C"

#ifdef FRAME_RANGE_SHIM_MAIN
#include <cstdio>
// a table of irregular blocks (some empty, offsets past 4 GiB), every range around every boundary, pass sizes 1 and 256 MiB
int main() {
    std::vector<uint64_t> co{0};
    std::vector<uint32_t> lw;
    uint64_t x = 88172645463325252ull;
    for (int b = 0; b < 400; b++) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        const uint64_t size = b % 7 == 3 ? 0 : (b == 5 ? 5ull << 30 : x % 70000);
        co.push_back(co.back() + size);
        lw.push_back((uint32_t)(x >> 40) % 65536u | (b % 3 == 0 ? STORED_BIT : 0u));
    }
    const uint32_t n = (uint32_t)lw.size();
    std::vector<uint64_t> off, len;
    for (uint32_t b = 0; b <= n; b++)
        for (int d = -1; d <= 1; d++)
            for (uint64_t l : {0ull, 1ull, 2ull, 70001ull, 6ull << 30}) {
                if (co[b] == 0 && d < 0) continue;
                off.push_back(co[b] + d); len.push_back(l);
            }
    const uint32_t m = (uint32_t)off.size();
    std::vector<uint64_t> per(4ull * m), out(5);
    uint64_t sum = 0;
    for (uint32_t r = 0; r < m; r++) { fr_locate(co.data(), lw.data(), n, off[r], len[r], out.data()); sum += out[0] + out[1] + out[2] + out[4]; }
    const uint32_t p1 = fr_plan(co.data(), lw.data(), n, off.data(), len.data(), m, nullptr, 1, per.data());
    const uint32_t p2 = fr_plan(co.data(), lw.data(), n, off.data(), len.data(), m, nullptr, 256ull << 20, per.data());
    std::printf("%u ranges, %u / %u passes, checksum %llu\n", m, p1, p2, (unsigned long long)sum);
    return 0;
}
#endif
