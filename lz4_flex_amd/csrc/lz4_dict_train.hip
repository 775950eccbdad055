// lz4_dict_train.hip -- lz4flex_dict_train: a dictionary cut from a batch of samples, on the device.  The rule is the one of
// tests/sim/dict_train_model.c (the definition; these kernels equal it byte for byte): the 8-byte windows ("candidates") of all samples
// are hashed to 20 bits and counted; a window weighs its hash's count unless one of the k - 1 windows in front of it in its sample has
// the same hash; a segment of k bytes scores the sum of its windows' weights; step t takes the best segment start of region t mod E
// of the global candidate numbers, sets the counters of its windows to 0 and puts its bytes in FRONT of what was taken before.
// The host knows neither the number of candidates nor E: the launch sequence depends on n, dict_cap and k alone --
//   memset           the header and the 2^20 counters
//   count            a lane takes 16 consecutive positions of a sample from 24 bytes read once (a 16-byte tile and the 8 bytes
//                    behind it), merges equal neighbours (runs of one byte put every window on one counter) and adds without a return value,
//                    through a combining cache in LDS that a workgroup flushes once
//   scan             lz4_packed.hip's three-phase exclusive scan over the candidates per sample: cstart[0 .. n], cstart[n] = total
//   setup            one lane: E, R, the capacity, the status (total >= 2^32: UNSUPPORTED), done
//   2 nseg x score   a workgroup per tile of SCORE_TILE global numbers of the step's region: the hashes of the tile and its halo (k - 1
//                    in front, k - 8 behind) once into LDS, first(p) by looking back through them, the weights from the counters, an
//                    LDS prefix sum, every start's score as a difference of two prefix values, ONE 64-bit atomicMax of
//                    score << 32 | ~(region-relative number) on the header's word -- nothing else is written;
//           commit   one workgroup: the winner's bytes to the staging area (filled from the back), its counters to 0, the capacity
//                    left, the run of steps without a winner, done, the word back to 0
//   finish           one workgroup: staging -> dict_out[0 .. dict_len), dict_len, status.
// Kernel boundaries on the one stream are the only ordering; a step behind `done` returns at once.  Every store is a plain vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4_copy_range.h"
#include "lz4_device.h"

namespace lz4flex_dev {

namespace {

constexpr uint32_t THREADS = 256u;
constexpr uint32_t FREQ_SLOTS = 1u << 20;
constexpr uint32_t W_MAX = FREQ_SLOTS - 1u;                      // a window's weight at most: a score stays below 2^31
constexpr uint32_t K_MAX = 2048u, CAP_MAX = 65536u;
constexpr uint32_t COUNT_TILE = THREADS * 16u;                   // positions per workgroup step of the count kernel
constexpr uint32_t COUNT_GRID = 2048u;
constexpr uint32_t CACHE_SLOTS = 8192u;                          // the count kernel's combining cache in LDS: (hash, count) pairs
constexpr uint32_t CACHE_EMPTY = 0xFFFFFFFFu;                    // (no hash: a hash has 20 bits)
constexpr uint32_t SCORE_TILE = 2048u;                           // segment starts per workgroup step
constexpr uint32_t SCORE_GRID = 512u;                            // the tiles of a region beyond it are strided over
constexpr uint32_t WGT_MAX = SCORE_TILE + K_MAX - 8u;            // windows whose weight a tile needs: its starts and k - 8 behind
constexpr uint32_t WIN_MAX = WGT_MAX + K_MAX - 1u;               // ... and whose hash: k - 1 more in front
constexpr uint32_t SCAN_PER = (WGT_MAX + THREADS - 1u) / THREADS;
constexpr uint32_t HSH_SLOTS = K_MAX - 1u + SCAN_PER * THREADS;  // (>= WIN_MAX: repeats reads, and drops, up to SCAN_PER * THREADS entries)
constexpr uint32_t TAG_SPAN = 4096u;                             // sample tags: 12 bits above the 20 of a hash
static_assert(HSH_SLOTS >= WIN_MAX, "the window fits");

struct TrainHdr {
    unsigned long long best;      // the step's argmax word; 0 = no start with a score above 0 yet
    uint64_t total;               // candidates in the batch
    uint32_t E, R;                // regions, candidates per region
    uint32_t remaining;           // capacity left: the staging area is filled down to here
    uint32_t zero_run;            // steps in a row without a winner
    uint32_t done;
    int32_t status;
};
constexpr size_t HDR_BYTES = 256u;
static_assert(sizeof(TrainHdr) <= HDR_BYTES, "the header has its own 256 bytes in front of the counters");

struct TrainWork {
    TrainHdr* hdr;
    uint32_t* freq;       // 2^20 counters
    uint64_t* size;       // n: candidates of sample i
    uint64_t* cstart;     // n + 1: their exclusive sums, cstart[n] = total
    uint64_t* tiles;      // the scan's tile sums
    uint8_t* staging;     // CAP_MAX bytes
};
TrainWork train_work(void* work, uint32_t n) {
    uint8_t* p = (uint8_t*)work;
    TrainWork w;
    w.hdr = (TrainHdr*)p; p += HDR_BYTES;
    w.freq = (uint32_t*)p; p += 4u * (size_t)FREQ_SLOTS;
    w.size = (uint64_t*)p; p += up256(8u * (size_t)n);
    w.cstart = (uint64_t*)p; p += up256(8u * ((size_t)n + 1u));
    w.tiles = (uint64_t*)p; p += up256(8u * scan_tiles(n));
    w.staging = p;
    return w;
}

__device__ __forceinline__ uint32_t hash8(uint64_t v) { return (uint32_t)((v * 0x9E3779B185EBCA87ull) >> 44); }
__device__ __forceinline__ uint64_t load8(const uint8_t* p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }   // (any alignment)

// the sample that holds global candidate number g < total: the largest i in [lo, hi] with cstart[i] <= g (its successor starts behind
// g, so it has candidates; samples without any share their neighbour's start and are passed over)
__device__ __forceinline__ uint32_t sample_of(const uint64_t* __restrict__ cstart, uint32_t lo, uint32_t hi, uint64_t g) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (cstart[mid] <= g) lo = mid; else hi = mid - 1u;
    }
    return lo;
}

// Bit j of the result: entry e = f0 + tid + 256 j of the window has an equal word among the k - 1 entries in front of it -- and, LIMIT,
// no further back than reach[e - f0].  A word is a hash with the tag of its sample (the sample's index counted from the window's first
// one, 12 bits) above it: while a window's samples span fewer than 4 096 indices, entries of different samples never compare equal, an
// entry of the same sample within k - 1 lies behind the sample's start by itself, and no limit is needed; a window that has its full
// halo in front never reads below 0 either.  The distance is the outer loop: every iteration issues SCAN_PER independent reads of
// consecutive words across the lanes, so that the look-back is bound by LDS throughput and not by a chain of read-compare-branch.
template <bool LIMIT>
__device__ __forceinline__ uint32_t repeats(const uint32_t* hsh, const uint16_t* reach, uint32_t f0, uint32_t k, uint32_t tid) {
    uint32_t h[SCAN_PER], lim[SCAN_PER], least[SCAN_PER];      // least[j]: the minimum of word ^ h[j] so far -- 0 once an equal word was seen
#pragma unroll
    for (uint32_t j = 0; j < SCAN_PER; ++j) {
        h[j] = hsh[f0 + tid + j * THREADS];
        lim[j] = LIMIT ? reach[tid + j * THREADS] : 0u;
        least[j] = 0xFFFFFFFFu;
    }
    for (uint32_t d = 1u; d < k; ++d) {
#pragma unroll
        for (uint32_t j = 0; j < SCAN_PER; ++j) {
            const uint32_t e = f0 + tid + j * THREADS;
            uint32_t diff;
            if (LIMIT) diff = d <= lim[j] ? hsh[e >= d ? e - d : 0u] ^ h[j] : 0xFFFFFFFFu;
            else diff = hsh[e - d] ^ h[j];
            least[j] = diff < least[j] ? diff : least[j];
        }
    }
    uint32_t bits = 0u;
#pragma unroll
    for (uint32_t j = 0; j < SCAN_PER; ++j) bits |= (uint32_t)(least[j] == 0u) << j;
    return bits;
}

}  // namespace

__global__ void __launch_bounds__(256) dict_train_count_kernel(const uint8_t* __restrict__ in_base, const uint64_t* __restrict__ in_off,
                                                               const uint32_t* __restrict__ in_len, uint32_t n, uint32_t* __restrict__ freq,
                                                               uint64_t* __restrict__ size) {
    // Adds to the 4 MiB table are served at the memory side, one request per lane; a workgroup collects what it can in LDS first.  A
    // slot belongs to the first hash that claims it for the life of the workgroup; a hash that finds its slot taken goes to the table
    // directly.  The sums are the same whichever way an add takes.
    __shared__ uint32_t ckey[CACHE_SLOTS], ccnt[CACHE_SLOTS];
    for (uint32_t sl = threadIdx.x; sl < CACHE_SLOTS; sl += THREADS) { ckey[sl] = CACHE_EMPTY; ccnt[sl] = 0u; }
    __syncthreads();
    auto add = [&](uint32_t h, uint32_t by) {
        const uint32_t sl = h & (CACHE_SLOTS - 1u);
        const uint32_t owner = atomicCAS(&ckey[sl], CACHE_EMPTY, h);
        if (owner == CACHE_EMPTY || owner == h) atomicAdd(&ccnt[sl], by);
        else atomicAdd(&freq[h], by);
    };
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint32_t len = in_len[i];
        const uint32_t c = len >= 8u ? len - 7u : 0u;
        if (blockIdx.y == 0u && threadIdx.x == 0u) size[i] = c;
        const uint8_t* src = in_base + in_off[i];
        for (uint64_t base = (uint64_t)blockIdx.y * COUNT_TILE; base < c; base += (uint64_t)gridDim.y * COUNT_TILE) {
            const uint64_t p0 = base + threadIdx.x * 16u;                  // this lane's positions: p0 .. p0 + 15
            if (p0 >= c) continue;
            uint64_t w0 = 0ull, w1 = 0ull, w2 = 0ull;                        // sample[p0 .. p0 + 24), zeros behind the sample's end
            if (p0 + 24u <= len) {
                w0 = load8(src + p0); w1 = load8(src + p0 + 8u); w2 = load8(src + p0 + 16u);
            } else {
#pragma unroll
                for (uint32_t b = 0; b < 24u; ++b) {
                    const uint64_t v = p0 + b < len ? (uint64_t)src[p0 + b] << (8u * (b & 7u)) : 0ull;
                    if (b < 8u) w0 |= v; else if (b < 16u) w1 |= v; else w2 |= v;
                }
            }
            const uint32_t m = c - p0 < 16u ? (uint32_t)(c - p0) : 16u;    // the positions that are candidates
            uint32_t cur = hash8(w0), run = 1u;
#pragma unroll
            for (uint32_t j = 1u; j < 16u; ++j) {
                if (j >= m) break;
                const uint32_t sh = 8u * (j & 7u);
                const uint64_t a = j < 8u ? w0 : w1, b = j < 8u ? w1 : w2;
                const uint32_t h = hash8(sh ? (a >> sh) | (b << (64u - sh)) : a);
                if (h == cur) { ++run; continue; }
                add(cur, run);
                cur = h; run = 1u;
            }
            add(cur, run);
        }
    }
    __syncthreads();
    for (uint32_t sl = threadIdx.x; sl < CACHE_SLOTS; sl += THREADS)
        if (ccnt[sl] != 0u) atomicAdd(&freq[ckey[sl]], ccnt[sl]);
}

__global__ void dict_train_setup_kernel(const uint64_t* __restrict__ cstart, uint32_t n, uint32_t cap, uint32_t k, TrainHdr* __restrict__ hdr) {
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    const uint64_t total = cstart[n];
    const uint32_t nseg = (cap + k - 1u) / k;
    uint64_t E = total / (4ull * k);
    if (E > nseg) E = nseg;
    if (E < 1ull) E = 1ull;
    const bool too_many = (total >> 32) != 0ull;
    hdr->best = 0ull;
    hdr->total = total;
    hdr->E = (uint32_t)E;
    hdr->R = too_many ? 0u : (uint32_t)((total + E - 1ull) / E);
    hdr->remaining = cap;
    hdr->zero_run = 0u;
    hdr->status = too_many ? LZ4FLEX_DEV_E_UNSUPPORTED : 0;
    hdr->done = too_many || total == 0ull ? 1u : 0u;
}

__global__ void __launch_bounds__(256) dict_train_score_kernel(const uint8_t* __restrict__ in_base, const uint64_t* __restrict__ in_off,
                                                               const uint64_t* __restrict__ cstart, uint32_t n,
                                                               const uint32_t* __restrict__ freq, TrainHdr* __restrict__ hdr, uint32_t k,
                                                               uint32_t t) {
    __shared__ uint32_t hsh[HSH_SLOTS];                  // the window's hashes, each with its sample's tag above bit 20
    __shared__ uint32_t pre[WGT_MAX + 1u];               // weights, then their prefix sums (mod 2^32: a score is a difference below 2^31)
    __shared__ uint16_t reach[SCAN_PER * THREADS];       // how far first(p) looks back: min(p, k - 1)
    __shared__ uint16_t ext[SCORE_TILE];                 // the windows of the segment at a start: min(c - p, k - 7)
    __shared__ unsigned long long red[THREADS];
    __shared__ uint32_t part[THREADS];
    __shared__ uint32_t span[2];
    if (hdr->done) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t total = hdr->total;
    const uint32_t R = hdr->R;
    const uint64_t lo = (uint64_t)(t % hdr->E) * R;
    const uint64_t hi = lo + R < total ? lo + R : total;
    if (lo >= hi) return;
    const uint64_t n_tiles = (hi - lo + SCORE_TILE - 1u) / SCORE_TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t g0 = lo + tile * SCORE_TILE;
        const uint64_t g1 = g0 + SCORE_TILE < hi ? g0 + SCORE_TILE : hi;
        const uint32_t f0 = g0 < k - 1u ? (uint32_t)g0 : k - 1u;          // halo in front
        const uint64_t wlo = g0 - f0;
        const uint64_t whi = g1 + (k - 8u) < total ? g1 + (k - 8u) : total;
        const uint32_t W = (uint32_t)(whi - wlo), nw = W - f0, ns = (uint32_t)(g1 - g0);
        if (tid == 0u) {
            span[0] = sample_of(cstart, 0u, n - 1u, wlo);
            span[1] = sample_of(cstart, span[0], n - 1u, whi - 1u);
        }
        __syncthreads();
        const uint32_t i_lo = span[0], i_hi = span[1];
        for (uint32_t e = tid; e < W; e += THREADS) {
            const uint64_t g = wlo + e;
            const uint32_t i = sample_of(cstart, i_lo, i_hi, g);
            const uint64_t cs = cstart[i];
            const uint32_t p = (uint32_t)(g - cs), c = (uint32_t)(cstart[i + 1u] - cs);
            hsh[e] = hash8(load8(in_base + in_off[i] + p)) | ((i - i_lo) & (TAG_SPAN - 1u)) << 20;
            if (e >= f0) {
                reach[e - f0] = (uint16_t)(p < k - 1u ? p : k - 1u);
                if (e - f0 < ns) ext[e - f0] = (uint16_t)(c - p < k - 7u ? c - p : k - 7u);
            }
        }
        if (tid == 0u) pre[0] = 0u;
        __syncthreads();
        // first(p) for this thread's entries x = tid + 256 j; the common case needs no limit per entry (see repeats)
        const bool plain = f0 == k - 1u && i_hi - i_lo < TAG_SPAN;
        const uint32_t seen = plain ? repeats<false>(hsh, reach, f0, k, tid) : repeats<true>(hsh, reach, f0, k, tid);
#pragma unroll
        for (uint32_t j = 0; j < SCAN_PER; ++j) {
            const uint32_t x = tid + j * THREADS;
            if (x >= nw) break;
            uint32_t w = 0u;
            if (!((seen >> j) & 1u)) { w = freq[hsh[f0 + x] & (FREQ_SLOTS - 1u)]; w = w < W_MAX ? w : W_MAX; }
            pre[x + 1u] = w;
        }
        __syncthreads();
        // inclusive sums of pre[1 .. nw]: a contiguous share per thread, the shares' sums scanned across the workgroup
        const uint32_t a = 1u + tid * SCAN_PER, b = a + SCAN_PER < nw + 1u ? a + SCAN_PER : nw + 1u;
        uint32_t s = 0u;
        for (uint32_t x = a; x < b; ++x) s += pre[x];
        part[tid] = s;
        __syncthreads();
        for (uint32_t d = 1u; d < THREADS; d <<= 1) {
            const uint32_t u = tid >= d ? part[tid - d] : 0u;
            __syncthreads();
            part[tid] += u;
            __syncthreads();
        }
        uint32_t o = part[tid] - s;
        for (uint32_t x = a; x < b; ++x) { o += pre[x]; pre[x] = o; }
        __syncthreads();
        unsigned long long best = 0ull;
        for (uint32_t x = tid; x < ns; x += THREADS) {
            const uint32_t score = pre[x + ext[x]] - pre[x];
            const unsigned long long key = ((unsigned long long)score << 32) | (0xFFFFFFFFu - (uint32_t)(g0 + x - lo));
            if (score != 0u && key > best) best = key;
        }
        red[tid] = best;
        __syncthreads();
        for (uint32_t d = THREADS / 2u; d != 0u; d >>= 1) {
            if (tid < d && red[tid + d] > red[tid]) red[tid] = red[tid + d];
            __syncthreads();
        }
        if (tid == 0u && red[0] != 0ull) atomicMax(&hdr->best, red[0]);
        __syncthreads();                                 // (the next tile writes the arrays again)
    }
}

__global__ void __launch_bounds__(256) dict_train_commit_kernel(const uint8_t* __restrict__ in_base, const uint64_t* __restrict__ in_off,
                                                                const uint32_t* __restrict__ in_len, const uint64_t* __restrict__ cstart,
                                                                uint32_t n, uint32_t* __restrict__ freq, TrainHdr* __restrict__ hdr,
                                                                uint8_t* __restrict__ staging, uint32_t k, uint32_t t) {
    __shared__ uint32_t winner;
    if (hdr->done) return;
    const uint32_t tid = threadIdx.x;
    const unsigned long long word = hdr->best;
    const uint32_t E = hdr->E, R = hdr->R, remaining = hdr->remaining, zero_run = hdr->zero_run;
    __syncthreads();                                     // (every lane has read the header before lane 0 writes it)
    if (word == 0ull) {                                  // nothing scored above 0
        if (tid == 0u) { hdr->zero_run = zero_run + 1u; if (zero_run + 1u >= E) hdr->done = 1u; }
        return;
    }
    const uint64_t g = (uint64_t)(t % E) * R + (0xFFFFFFFFu - (uint32_t)word);
    if (tid == 0u) winner = sample_of(cstart, 0u, n - 1u, g);
    __syncthreads();
    const uint32_t i = winner;
    const uint32_t s = (uint32_t)(g - cstart[i]), len = in_len[i], c = len - 7u;
    const uint32_t L = len - s < k ? len - s : k;
    const uint32_t take = L < remaining ? L : remaining;
    const uint8_t* src = in_base + in_off[i];
    copy_range(staging + (remaining - take), src + s, take, tid, THREADS);
    const uint64_t pe = (uint64_t)s + (k - 7u) < c ? (uint64_t)s + (k - 7u) : c;
    for (uint64_t p = (uint64_t)s + tid; p < pe; p += THREADS) freq[hash8(load8(src + p))] = 0u;
    if (tid == 0u) {
        hdr->remaining = remaining - take;
        hdr->zero_run = 0u;
        hdr->best = 0ull;
        if (remaining == take) hdr->done = 1u;
    }
}

__global__ void __launch_bounds__(256) dict_train_finish_kernel(const TrainHdr* __restrict__ hdr, const uint8_t* __restrict__ staging, uint32_t cap,
                                                                uint8_t* __restrict__ dict_out, uint32_t* __restrict__ dict_len,
                                                                int32_t* __restrict__ status) {
    const uint32_t remaining = hdr->remaining;
    copy_range(dict_out, staging + remaining, cap - remaining, threadIdx.x, THREADS);
    if (threadIdx.x == 0u) { *dict_len = cap - remaining; *status = hdr->status; }
}

__global__ void dict_train_empty_kernel(uint32_t* __restrict__ dict_len, int32_t* __restrict__ status) {
    if (blockIdx.x == 0u && threadIdx.x == 0u) { *dict_len = 0u; *status = 0; }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
size_t dict_train_work_bytes(uint32_t n) {
    return HDR_BYTES + 4u * (size_t)FREQ_SLOTS + up256(8u * (size_t)n) + up256(8u * ((size_t)n + 1u)) + up256(8u * scan_tiles(n)) + CAP_MAX;
}

hipError_t launch_dict_train(const uint8_t* in_base, const uint64_t* in_off, const uint32_t* in_len, uint32_t n, uint8_t* dict_out,
                             uint32_t dict_cap, uint32_t k, uint32_t* dict_len, int32_t* status, void* work, hipStream_t s) {
    if (n == 0u || dict_cap == 0u) {
        hipLaunchKernelGGL(dict_train_empty_kernel, dim3(1), dim3(1), 0, s, dict_len, status);
        return hipGetLastError();
    }
    if (k < 64u || k > K_MAX || dict_cap > CAP_MAX) return hipErrorInvalidValue;
    const TrainWork w = train_work(work, n);
    hipError_t e = hipMemsetAsync(work, 0, HDR_BYTES + 4u * (size_t)FREQ_SLOTS, s);
    if (e != hipSuccess) return e;
    const uint32_t gx = n < COUNT_GRID ? n : COUNT_GRID;
    hipLaunchKernelGGL(dict_train_count_kernel, dim3(gx, COUNT_GRID / gx), dim3(THREADS), 0, s, in_base, in_off, in_len, n, w.freq, w.size);
    if ((e = launch_packed_scan(w.size, n, 1u, ~0ull, 0u, w.tiles, w.cstart, nullptr, nullptr, nullptr, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(dict_train_setup_kernel, dim3(1), dim3(1), 0, s, (const uint64_t*)w.cstart, n, dict_cap, k, w.hdr);
    const uint32_t steps = 2u * ((dict_cap + k - 1u) / k);
    for (uint32_t t = 0; t < steps; ++t) {
        hipLaunchKernelGGL(dict_train_score_kernel, dim3(SCORE_GRID), dim3(THREADS), 0, s, in_base, in_off, (const uint64_t*)w.cstart, n,
                           (const uint32_t*)w.freq, w.hdr, k, t);
        hipLaunchKernelGGL(dict_train_commit_kernel, dim3(1), dim3(THREADS), 0, s, in_base, in_off, in_len, (const uint64_t*)w.cstart, n, w.freq,
                           w.hdr, w.staging, k, t);
    }
    hipLaunchKernelGGL(dict_train_finish_kernel, dim3(1), dim3(THREADS), 0, s, (const TrainHdr*)w.hdr, (const uint8_t*)w.staging, dict_cap, dict_out,
                       dict_len, status);
    return hipGetLastError();
}

}  // namespace lz4flex_dev
