// lz4_host_stage.h -- how a MEM_HOST call of the C ABI mirrors the caller's host layout on the device (capi.cpp: every batched entry
// point that takes LZ4FLEX_MEM_HOST).  Host only, no kernel includes it.  Its layers:
//   ColumnPlan  pure arithmetic (no HIP header: tests/sim/ compiles it with g++ under LZ4FLEX_STAGE_PLAN_ONLY): the descriptor and result
//               COLUMNS of a call, one image that a host buffer and device memory share -- the frame layer's Desc (lz4_ctx.h) is one too;
//   StagePlan   the columns and the REGIONS of the arena, the column image among them;
//   HostStage   the plan bound to a context's page-locked buffer, its arena and its stream (capi.cpp stage_open grows the two buffers):
//               typed views of the columns on either side, the fillers, the transfers.
// The rule every path follows: the caller's offsets are rebased onto the span they cover (fill_offsets), the span goes up into a region
// of its own, the `up` columns go up in ONE transfer, the call's launches run on device views of all this -- the code a MEM_DEVICE call
// runs -- and the `down` columns come back in ONE transfer.  What a path adds to that is in capi.cpp, next to its launches.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#ifndef LZ4FLEX_STAGE_PLAN_ONLY
#include <hip/hip_runtime.h>
#endif

namespace lz4flex_dev {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// arrays laid out one behind the other, each start aligned: the layout a pinned host mirror and its device copy share
struct Layout {
    size_t align;
    size_t end = 0;               // the bytes taken so far (aligned)
    size_t take(size_t bytes) { const size_t at = end; end = align_up(end + bytes, align); return at; }
};

template <class T> struct Col { size_t at, count; };      // `count` elements at byte `at` of the column image
struct Region { size_t at, bytes, room; };                // `bytes` at byte `at` of the arena; the next region starts `room` behind it

// The columns of one image, declared in the caller's order: every up() before every down().  A column of 0 elements shares its start
// with its neighbour and is never touched.  The one column arithmetic of the host layer: StagePlan (below) and Desc (lz4_ctx.h) are
// column plans, frame_cols.h names the frame layer's columns over one.
struct ColumnPlan {
    Layout cols;
    size_t up_bytes = 0;          // what the device reads lies in front of this, what it only writes behind
    explicit ColumnPlan(size_t align = 16) : cols{align} {}
    template <class T> Col<T> up(size_t count) { const Col<T> c{cols.take(sizeof(T) * count), count}; up_bytes = cols.end; return c; }
    template <class T> Col<T> down(size_t count) { return Col<T>{cols.take(sizeof(T) * count), count}; }
    size_t total() const { return cols.end; }
    template <class T> size_t from(Col<T> c) const { return cols.end - c.at; }      // from this down column to the end
    // the column in memory that holds the image at `base` (device scratch that has no host image: frame_index.cpp index_build)
    template <class T> static T* view(void* base, Col<T> c) { return reinterpret_cast<T*>(static_cast<uint8_t*>(base) + c.at); }
};

// The columns and, in their order in the arena, the regions; columns() among them once the last column is declared.
struct StagePlan : ColumnPlan {
    size_t arena_end = 0, arena_bytes = 256;
    Region desc{0, 0, 0};         // where the column image lies in the arena
    explicit StagePlan(size_t align = 16) : ColumnPlan(align) {}
    // a region starts at a multiple of 256.  slack: the kernels read whole dwords / 16-byte units behind a region's last byte (the data
    // regions take 64); the 256 bytes behind the last region's last byte keep the same reads inside the allocation
    Region region(size_t bytes, size_t slack) {
        const Region r{arena_end, bytes, align_up(bytes + slack, 256)};
        arena_end += r.room;
        arena_bytes = r.at + bytes + 256;
        return r;
    }
    Region columns(size_t slack = 0) { return desc = region(total(), slack); }
};

#ifndef LZ4FLEX_STAGE_PLAN_ONLY
struct HostStage : StagePlan {
    uint8_t* hp = nullptr;        // the column image in page-locked memory
    uint8_t* d = nullptr;         // the arena
    hipStream_t s = nullptr;
    using StagePlan::StagePlan;
    template <class T> T* host(Col<T> c) const { return reinterpret_cast<T*>(hp + c.at); }
    template <class T> T* dev(Col<T> c) const { return reinterpret_cast<T*>(d + desc.at + c.at); }
    template <class T> T* dev_opt(Col<T> c) const { return c.count ? dev(c) : nullptr; }      // an optional array the call came without
    uint8_t* dev(const Region& r) const { return d + r.at; }
    // the caller's offsets, rebased onto the span that starts at `lo` (only_where: 0 where that array holds 0 -- the offset is not looked at)
    void fill_offsets(Col<uint64_t> c, const uint64_t* off, uint64_t lo, const uint32_t* only_where = nullptr) const {
        uint64_t* h = host(c);
        for (size_t i = 0; i < c.count; i++) h[i] = only_where && !only_where[i] ? 0u : off[i] - lo;
    }
    template <class T, class U> void fill(Col<T> c, const U* src) const {
        static_assert(sizeof(T) == sizeof(U), "a column takes its caller's array as it is");
        if (c.count) memcpy(hp + c.at, src, sizeof(T) * c.count);
    }
    template <class T> void zero(Col<T> c) const { if (c.count) memset(hp + c.at, 0, sizeof(T) * c.count); }
    template <class T, class U> void read(Col<T> c, U* dst, size_t count) const {
        static_assert(sizeof(T) == sizeof(U), "a column is copied to its caller's array as it is");
        memcpy(dst, hp + c.at, sizeof(T) * count);
    }
    template <class T, class U> void read(Col<T> c, U* dst) const { read(c, dst, c.count); }
    hipError_t send(const Region& r, const void* src, size_t bytes) const {
        return bytes ? hipMemcpyAsync(d + r.at, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    }
    hipError_t send(const Region& r, const void* src) const { return send(r, src, r.bytes); }
    hipError_t send_columns() const { return hipMemcpyAsync(d + desc.at, hp, up_bytes, hipMemcpyHostToDevice, s); }
    template <class T> hipError_t fetch_columns(Col<T> first) const {
        return hipMemcpyAsync(hp + first.at, d + desc.at + first.at, from(first), hipMemcpyDeviceToHost, s);
    }
};
#endif

}  // namespace lz4flex_dev
