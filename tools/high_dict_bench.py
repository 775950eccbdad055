#!/usr/bin/env python3
"""compress_mode 2 ("high") against ONE 32 KiB dictionary ("compress_high_dict" 1) next to the other encoders with the same
dictionary, on device-resident batches, one session.  The legs ALTERNATE: each round times one call of every leg with device events,
after --warmup rounds; the median, minimum and maximum of --reps rounds are reported per leg.

  shapes  (a) 16 384 x 64 KiB JSON tiles, one 32 KiB JSON dictionary   (b) 65 536 x 4 KiB log records, one 32 KiB dictionary of other
          log lines   (the workloads of tools/dict_bench.py)
  legs    mode 0 and mode 1 through lz4flex_compress_batch_shared_dict; mode 2 at depths 4, 16 and 64 through the shared entry with
          "compress_high_digest" 1 and 0 and through lz4flex_compress_batch_ex; mode 2 at depth 16 WITHOUT the dictionary, for scale

After the loop the three mode 2 legs of a depth are compared byte for byte on the device, and every block of every distinct output is
decoded by the oracle's decoder (with the dictionary) and compared with its input.

usage: python tools/high_dict_bench.py [--reps 3] [--warmup 1] [--workload a|b|both] [--scale 1.0]   (one JSON line per leg)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dict_bench import p, workload  # noqa: E402
from lz4_flex_amd import _lib as L  # noqa: E402

# leg: (compress_mode, compress_depth, entry, compress_high_digest)
LEGS = {"mode 0, dictionary": (0, None, "shared", 1), "mode 1, dictionary": (1, None, "shared", 1)}
for _d in (4, 16, 64):
    LEGS["mode 2 depth %d, shared, digest" % _d] = (2, _d, "shared", 1)
    LEGS["mode 2 depth %d, shared, joint sort" % _d] = (2, _d, "shared", 0)
    LEGS["mode 2 depth %d, _ex" % _d] = (2, _d, "ex", 1)
LEGS["mode 2 depth 16, no dictionary"] = (2, 16, "plain", 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", choices=["a", "b", "both"], default="both")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of every workload's blocks")
    args = ap.parse_args()
    import oracle_api as O
    lib = L.load()
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), -1) == 0
    assert lib.lz4flex_set_tuning(ctx, b"compress_high_dict", 1) == 0
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    for w in (["b", "a"] if args.workload == "both" else [args.workload]):
        what, src, dic, n, blk = workload(w, dev)
        n = max(1, int(n * args.scale))
        src = src[:n * blk]
        in_off = torch.arange(n, dtype=torch.int64, device=dev) * blk
        in_len = torch.full((n,), blk, dtype=torch.int32, device=dev)
        cap1 = 20 + blk * 110 // 100
        out_off = torch.arange(n, dtype=torch.int64, device=dev) * cap1
        out_cap = torch.full((n,), cap1, dtype=torch.int32, device=dev)
        d_off = torch.zeros(n, dtype=torch.int64, device=dev)
        d_len = torch.full((n,), dic.numel(), dtype=torch.int32, device=dev)
        ext = L.CompressExt(dic.data_ptr(), d_off.data_ptr(), d_len.data_ptr())
        bufs = {leg: (torch.zeros(n * cap1, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                      torch.full((n,), -1, dtype=torch.int32, device=dev)) for leg in LEGS}

        def once(leg):
            mode, depth, entry, digest = LEGS[leg]
            out, out_len, status = bufs[leg]
            assert lib.lz4flex_set_tuning(ctx, b"compress_mode", mode) == 0
            assert lib.lz4flex_set_tuning(ctx, b"compress_high_digest", digest) == 0
            if depth:
                assert lib.lz4flex_set_tuning(ctx, b"compress_depth", depth) == 0
            tail = (p(out), p(out_off), p(out_cap), p(out_len), p(status))
            if entry == "ex":
                rc = lib.lz4flex_compress_batch_ex(ctx, p(src), p(in_off), p(in_len), None, n, *tail, C.byref(ext), L.MEM_DEVICE, sp)
            elif entry == "shared":
                rc = lib.lz4flex_compress_batch_shared_dict(ctx, p(src), p(in_off), p(in_len), n, *tail, p(dic), dic.numel(), L.MEM_DEVICE, sp)
            else:
                rc = lib.lz4flex_compress_batch(ctx, p(src), p(in_off), p(in_len), None, n, *tail, L.MEM_DEVICE, sp)
            assert rc == 0, (rc, L.last_error())

        times = {leg: [] for leg in LEGS}
        for r in range(args.warmup + args.reps):
            for leg in LEGS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                once(leg)
                e1.record(stream)
                e1.synchronize()
                if r >= args.warmup:
                    times[leg].append(e0.elapsed_time(e1))
        host, hdic = src.cpu().numpy(), dic.cpu().numpy().tobytes()
        decoded = {}
        for leg, (mode, depth, entry, digest) in LEGS.items():
            out, out_len, status = bufs[leg]
            assert int((status != 0).sum()) == 0, (leg, "compress status")
            same_as = "mode 2 depth %d, shared, digest" % depth if mode == 2 and entry != "plain" and not (entry == "shared" and digest) else None
            if same_as:
                decoded[leg] = bool(torch.equal(out_len, bufs[same_as][1])) and bool(torch.equal(out, bufs[same_as][0]))
                assert decoded[leg], (leg, "bytes differ from the digest leg's")
                continue
            h_out, h_len = out.cpu().numpy(), out_len.cpu().numpy()
            for k in range(n):
                got = h_out[k * cap1:k * cap1 + int(h_len[k])].tobytes()
                assert O.decompress(got, blk, dict_data=None if entry == "plain" else hdic) == ("ok", host[k * blk:(k + 1) * blk].tobytes()), (leg, k)
            decoded[leg] = True
        for leg in LEGS:
            ms = statistics.median(times[leg])
            total = int(bufs[leg][1].to(torch.int64).sum())
            print(json.dumps({"workload": w, "what": what, "blocks": n, "leg": leg, "ms": round(ms, 3), "ms_min": round(min(times[leg]), 3),
                              "ms_max": round(max(times[leg]), 3), "ratio": round(total / (n * blk), 4), "bytes": total,
                              "decoded_by_the_oracle_or_equal_to_the_digest_leg": decoded[leg]}), flush=True)
        del src, bufs
        torch.cuda.empty_cache()
    lib.lz4flex_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
