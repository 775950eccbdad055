#!/usr/bin/env python3
"""tools/frame_range_bench.py -- the frame index and range reads through it next to a full decode of the same frame, on device-resident
Independent frames (the buffers are torch tensors, every codec call goes through ctypes as in tools/partial_bench.py).

  frames    json      --gib GiB of 64 KiB JSON tiles, Max64KB blocks            (workloads.json_tiles)
            json_sums the same with block checksums
            log       --gib GiB of log lines, Max4MB blocks                     (workloads.log_stream)
  legs      create       lz4flex_frame_index_create (blocks until the index exists)
            walk, scan   its two long launches alone, through lz4flex_frame_walk_device and lz4flex_decompressed_size_batch on the index's
                         own tables (the offset scan has no entry of its own: create minus these two is the rest)
            1x1M, 16x1M, 1024x4K, 65536x4K   lz4flex_frame_read_ranges of that many ranges at random offsets
            whole        the whole content as one range
            full         lz4flex_frame_decompress_many with n = 1: what a caller without the index has to do for any of the above
            json_sums runs 16x1M and whole with "frame_range_checksums" 1 and 0
Every call blocks until its work is done, so a leg is a host clock around the call between two device synchronisations.  The legs
ALTERNATE inside one session; the median, minimum and maximum of --reps rounds after --warmup rounds are reported, one JSON line per
leg, and every leg's output is compared with the source once.

usage: python tools/frame_range_bench.py [--gib 1] [--reps 5] [--warmup 1] [--frames json json_sums log]"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MIB = 1 << 20


def u64(v):
    return (C.c_uint64 * max(len(v), 1))(*v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", nargs="+", default=["json", "json_sums", "log"], choices=["json", "json_sums", "log"])
    args = ap.parse_args()
    import torch
    import oracle_api as O
    from lz4_flex_amd import _lib as L, frame as F, workloads
    lib = L.load()
    assert lib.lz4flex_device_count() >= 1, "no GPU: nothing here is measured without one"
    dev = torch.device("cuda", 0)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())     # noqa: E731
    total = int(args.gib * (1 << 30)) // (4 * MIB) * (4 * MIB)
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for name in args.frames:
        if name == "log":
            src = workloads.log_stream(0, total, device=dev)
            info = F.FrameInfo(block_size=F.BlockSize.Max4MB)
        else:
            src = workloads.json_tiles(O.fixture_plain("compression_66k_JSON"), total, device=dev)
            info = F.FrameInfo(block_size=F.BlockSize.Max64KB, block_checksums=name == "json_sums")
        fi = info._c()
        cap = int(lib.lz4flex_frame_compress_bound(total, C.byref(fi)))
        buf = torch.empty(cap, dtype=torch.uint8, device=dev)
        flen, fst = (C.c_uint64 * 1)(), (C.c_int32 * 1)()
        assert lib.lz4flex_frame_compress_many(ctx, p(src), u64([0]), u64([total]), 1, C.byref(fi), p(buf), u64([0]), u64([cap]), flen, fst,
                                               L.MEM_DEVICE, sp) == 0 and fst[0] == 0, L.last_error()
        frame_len = int(flen[0])
        frame = buf[:frame_len].clone()
        del buf
        h = C.c_void_p()
        assert lib.lz4flex_frame_index_create(ctx, p(frame), frame_len, L.MEM_DEVICE, C.byref(h), None) == 0, L.last_error()
        nblk = int(lib.lz4flex_frame_index_blocks(h))
        assert int(lib.lz4flex_frame_index_content_size(h)) == total
        po, lw = (C.c_uint64 * nblk)(), (C.c_uint32 * nblk)()
        assert lib.lz4flex_frame_index_table(h, None, po, lw) == 0
        d_po = torch.tensor(list(po), dtype=torch.int64, device=dev)
        d_len = torch.tensor([w & 0x7FFFFFFF for w in lw], dtype=torch.int32, device=dev)
        d_size, d_st = torch.zeros(nblk, dtype=torch.int64, device=dev), torch.zeros(nblk, dtype=torch.int32, device=dev)
        w_po, w_lw, w_info = torch.zeros(nblk + 8, dtype=torch.int64, device=dev), torch.zeros(nblk + 8, dtype=torch.int32, device=dev), \
            torch.zeros(4, dtype=torch.int32, device=dev)
        hdr_len = int(po[0]) - 4
        bs = 4 * MIB if name == "log" else 65536
        rnd = random.Random(1)
        shapes = {"1x1M": (1, MIB), "16x1M": (16, MIB), "1024x4K": (1024, 4096), "65536x4K": (65536, 4096), "whole": (1, total)}
        out = torch.empty(max([total] + [m * n for m, n in shapes.values()]), dtype=torch.uint8, device=dev)   # (every leg's ranges back to back)
        plans = {}
        for leg, (m, n) in shapes.items():
            assert n <= total and m * n <= out.numel(), leg
            offs = [0] if leg == "whole" else [rnd.randrange(total - n + 1) for _ in range(m)]
            plans[leg] = (offs, u64(offs), u64([n] * m), u64([i * n for i in range(m)]), (C.c_uint64 * m)(), (C.c_int32 * m)(), m, n)

        def read(leg):
            offs, ro, rl, oo, ol, st, m, n = plans[leg]
            assert lib.lz4flex_frame_read_ranges(ctx, h, p(frame), ro, rl, m, p(out), oo, ol, st, None, L.MEM_DEVICE, sp) == 0, L.last_error()

        def check(leg):
            offs, ro, rl, oo, ol, st, m, n = plans[leg]
            assert not any(st) and all(v == n for v in ol), leg
            for i in ([0] if m == 1 else rnd.sample(range(m), 8)):
                assert torch.equal(out[i * n:(i + 1) * n], src[offs[i]:offs[i] + n]), (leg, i)

        def create():
            x = C.c_void_p()
            assert lib.lz4flex_frame_index_create(ctx, p(frame), frame_len, L.MEM_DEVICE, C.byref(x), None) == 0
            lib.lz4flex_frame_index_free(x)

        def full():
            ol, st = (C.c_uint64 * 1)(), (C.c_int32 * 1)()
            assert lib.lz4flex_frame_decompress_many(ctx, p(frame), u64([0]), u64([frame_len]), 1, p(out), u64([0]), u64([total]), ol, st, None,
                                                     L.MEM_DEVICE, sp) == 0 and st[0] == 0 and ol[0] == total, L.last_error()

        legs = {"create": create,
                "walk": lambda: lib.lz4flex_frame_walk_device(p(frame), frame_len, hdr_len, int(name == "json_sums"), bs, nblk + 8, p(w_po), p(w_lw),
                                                              p(w_info), sp),
                "scan": lambda: lib.lz4flex_decompressed_size_batch(ctx, p(frame), p(d_po), p(d_len), nblk, None, p(d_size), p(d_st), L.MEM_DEVICE, sp),
                "full": full}
        for leg in shapes:
            legs[leg] = (lambda leg=leg: read(leg))
        if name == "json_sums":
            for leg in ("16x1M", "whole"):
                def unchecked(leg=leg):
                    assert lib.lz4flex_set_tuning(ctx, b"frame_range_checksums", 0) == 0
                    read(leg)
                    assert lib.lz4flex_set_tuning(ctx, b"frame_range_checksums", 1) == 0
                legs[leg + " sums off"] = unchecked
        for leg in shapes:                                            # every leg's bytes, once
            out.zero_()
            read(leg)
            torch.cuda.synchronize()
            check(leg)
        out.zero_()
        full()
        torch.cuda.synchronize()
        assert torch.equal(out[:total], src)
        times = {leg: [] for leg in legs}
        for rep in range(args.warmup + args.reps):
            for leg, fn in legs.items():
                t = timed(fn)
                if rep >= args.warmup:
                    times[leg].append(t)
        for leg, v in times.items():
            print(json.dumps({"frame": name, "content_bytes": total, "frame_bytes": frame_len, "blocks": nblk, "leg": leg,
                              "ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3),
                              "reps": len(v)}), flush=True)
        lib.lz4flex_frame_index_free(h)
        del src, frame, out
        torch.cuda.empty_cache()
    lib.lz4flex_ctx_destroy(ctx)
    return 0


if __name__ == "__main__":
    sys.exit(main())
