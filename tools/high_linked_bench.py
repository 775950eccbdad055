#!/usr/bin/env python3
"""compress_mode 2 ("high") over a stream's history ("compress_high_linked" 1) next to mode 0's Linked frames and mode 2's Independent
ones, on device-resident streams, one session.  The legs ALTERNATE: each round times one call of every leg (a frame call returns when
it has completed: wall clock around it; the raw batch: device events), after --warmup rounds; the median, minimum and maximum of --reps
rounds are reported per leg.

  shapes  (a) 256 streams x 4 MiB of log, blocks of 4 MiB   (b) the same streams, blocks of 64 KiB   (c) 4 096 streams x 256 KiB of log,
          blocks of 64 KiB -- all three through lz4flex_frame_compress_many   (d) a raw lz4flex_compress_batch of 16 384 x 64 KiB JSON
          tiles, each behind 32 KiB of the tile in front of it (LZ4FLEX_BLOCK_HISTORY)
  legs    mode 0 Linked; mode 2 Independent and mode 2 Linked at depths 4, 16 and 64   ((d): with / without the history flags)

After the loop every frame of every leg is decoded by the oracle's frame decoder and compared with its stream ((d): every block by the
oracle's block decoder, behind the bytes in front of it).

usage: python tools/high_linked_bench.py [--reps 3] [--warmup 1] [--shapes abcd] [--scale 1.0]   (one JSON line per leg)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from lz4_flex_amd import _lib as L, block, frame, workloads  # noqa: E402

# leg: (compress_mode, compress_depth, linked)
LEGS = {"mode 0, linked": ("fast", None, True)}
for _d in (4, 16, 64):
    LEGS["mode 2 depth %d, independent" % _d] = ("high", _d, False)
    LEGS["mode 2 depth %d, linked" % _d] = ("high", _d, True)

SHAPES = {"a": ("256 streams x 4 MiB log, blocks of 4 MiB", 256, 4 << 20, frame.BlockSize.Max4MB),
          "b": ("256 streams x 4 MiB log, blocks of 64 KiB", 256, 4 << 20, frame.BlockSize.Max64KB),
          "c": ("4096 streams x 256 KiB log, blocks of 64 KiB", 4096, 256 << 10, frame.BlockSize.Max64KB)}


def p(t):
    return C.c_void_p(t.data_ptr())


def setup(leg):
    mode, depth, _ = LEGS[leg]
    block.set_compress_mode(mode)
    if depth:
        block.set_compress_depth(depth)


def report(shape, what, n, leg, times, total, plain, ok):
    print(json.dumps({"shape": shape, "what": what, "streams": n, "leg": leg, "ms": round(statistics.median(times), 3), "ms_min": round(min(times), 3),
                      "ms_max": round(max(times), 3), "ratio": round(total / plain, 4), "bytes": total, "decoded_by_the_oracle": ok}), flush=True)


def frames_shape(shape, args, dev, O):
    what, n, size, bs = SHAPES[shape]
    n = max(1, int(n * args.scale))
    src = workloads.log_stream(0, n * size, device=dev)
    in_off, in_len = [k * size for k in range(n)], [size] * n
    lib = L.load()
    infos = {linked: frame.FrameInfo(block_size=bs, block_mode=frame.BlockMode.Linked if linked else frame.BlockMode.Independent) for linked in (True, False)}
    cap = int(lib.lz4flex_frame_compress_bound(size, C.byref(infos[True]._c())))
    out_off, out_cap = [k * cap for k in range(n)], [cap] * n
    bufs = {leg: torch.zeros(n * cap, dtype=torch.uint8, device=dev) for leg in LEGS}
    lens, times = {}, {leg: [] for leg in LEGS}
    for r in range(args.warmup + args.reps):
        for leg in LEGS:
            setup(leg)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lens[leg], st = frame.compress_frames_device(src, in_off, in_len, infos[LEGS[leg][2]], bufs[leg], out_off, out_cap)
            t1 = time.perf_counter()
            assert not any(st), (leg, "status")
            if r >= args.warmup:
                times[leg].append((t1 - t0) * 1e3)
    host = src.cpu().numpy()
    for leg in LEGS:
        h = bufs[leg].cpu().numpy()
        for k in range(n):
            f = h[k * cap:k * cap + lens[leg][k]].tobytes()
            assert O.frame_decompress(f, size)[:2] == (0, host[k * size:(k + 1) * size].tobytes()), (leg, k)
        report(shape, what, n, leg, times[leg], sum(lens[leg]), n * size, True)
    del src, bufs
    torch.cuda.empty_cache()


def raw_shape(args, dev, O):
    lib = L.load()
    n, blk, hist = max(2, int(16384 * args.scale)), 65536, 32768
    what = "raw batch, %d x 64 KiB JSON tiles, each behind 32 KiB of the tile in front of it" % n
    src = workloads.json_tiles(O.fixture_plain("compression_66k_JSON"), n * blk, device=dev)
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    in_off, in_len = ar * blk, torch.full((n,), blk, dtype=torch.int32, device=dev)
    cap1 = 20 + blk * 110 // 100
    out_off, out_cap = ar * cap1, torch.full((n,), cap1, dtype=torch.int32, device=dev)
    flags = torch.full((n,), hist << 8, dtype=torch.int32, device=dev)
    flags[0] = 0
    bufs = {leg: (torch.zeros(n * cap1, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                  torch.full((n,), -1, dtype=torch.int32, device=dev)) for leg in LEGS}
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    times = {leg: [] for leg in LEGS}
    for r in range(args.warmup + args.reps):
        for leg in LEGS:
            setup(leg)
            out, out_len, status = bufs[leg]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = lib.lz4flex_compress_batch(None, p(src), p(in_off), p(in_len), p(flags) if LEGS[leg][2] else None, n, p(out), p(out_off), p(out_cap),
                                            p(out_len), p(status), L.MEM_DEVICE, sp)
            e1.record(stream)
            e1.synchronize()
            assert rc == 0, (rc, L.last_error())
            if r >= args.warmup:
                times[leg].append(e0.elapsed_time(e1))
    host = src.cpu().numpy()
    for leg in LEGS:
        out, out_len, status = bufs[leg]
        assert int((status != 0).sum()) == 0, (leg, "compress status")
        h_out, h_len = out.cpu().numpy(), out_len.cpu().numpy()
        for k in range(n):
            got = h_out[k * cap1:k * cap1 + int(h_len[k])].tobytes()
            d = host[k * blk - hist:k * blk].tobytes() if LEGS[leg][2] and k else None
            assert O.decompress(got, blk, dict_data=d) == ("ok", host[k * blk:(k + 1) * blk].tobytes()), (leg, k)
        report("d", what, n, leg, times[leg], int(out_len.to(torch.int64).sum()), n * blk, True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="abcd")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of every shape's streams / blocks")
    args = ap.parse_args()
    import oracle_api as O
    dev = torch.device("cuda")
    block.set_compress_high_linked(True)
    try:
        for shape in args.shapes:
            if shape == "d":
                raw_shape(args, dev, O)
            else:
                frames_shape(shape, args, dev, O)
    finally:
        block.set_compress_mode("fast")
        block.set_compress_high_linked(False)


if __name__ == "__main__":
    main()
