"""tools/shared_dict_bench.py -- lz4flex_compress_batch_shared_dict next to lz4flex_compress_batch_ex with the same dictionary for every
block, on device-resident batches, compress_mode fast.  The legs ALTERNATE inside one session (per-block, shared, shared with
"compress_shared_dict" 0, per-block, ...): each round times one call of every leg with device events, after --warmup rounds; the
median, minimum and maximum of --reps rounds are reported per leg.  The outputs of all legs are compared byte for byte on the device
(so the ratio is the same number), the digest counter is read after the shared leg, and the shared leg's output is decoded by
lz4flex_decompress_batch_ex with the dictionary.

  (a) 16 384 x 64 KiB JSON tiles, one 32 KiB JSON dictionary     (b) 65 536 x 4 KiB log records, one 32 KiB dictionary of other log lines
  (the workloads of tools/dict_bench.py)

--prof (a -DLZ4FLEX_TOOLS -DLZ4W_PROF_STEPS build, selected with LZ4FLEX_LIB=<path>: python -m lz4_flex_amd.build --variant tools_prof
-DLZ4FLEX_TOOLS -DLZ4W_PROF_STEPS): one more call per leg with the encoder's cycle counters on -- where a window's cycles go, per
role (the counters of tools/wave_bench.py --prof; the timed numbers of such a build are not the product's).

usage: LZ4FLEX_TEST_HOOKS=1 python tools/shared_dict_bench.py [--reps 5] [--warmup 2] [--workload a|b|both] [--prof]   (one JSON line per leg)"""
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

from dict_bench import p, workload  # noqa: E402
from lz4_flex_amd import _lib as L  # noqa: E402

LEGS = ("per_block", "shared", "shared_off")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", choices=["a", "b", "both"], default="both")
    ap.add_argument("--prof", action="store_true")
    args = ap.parse_args()
    lib = L.load()
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), -1) == 0
    assert lib.lz4flex_set_tuning(ctx, b"compress_mode", 0) == 0
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    for w in (["a", "b"] if args.workload == "both" else [args.workload]):
        what, src, dic, n, blk = workload(w, dev)
        in_off = torch.arange(n, dtype=torch.int64, device=dev) * blk
        in_len = torch.full((n,), blk, dtype=torch.int32, device=dev)
        cap1 = 20 + blk * 110 // 100
        out_off = torch.arange(n, dtype=torch.int64, device=dev) * cap1
        out_cap = torch.full((n,), cap1, dtype=torch.int32, device=dev)
        d_off = torch.zeros(n, dtype=torch.int64, device=dev)
        d_len = torch.full((n,), dic.numel(), dtype=torch.int32, device=dev)
        ext = L.CompressExt(dic.data_ptr(), d_off.data_ptr(), d_len.data_ptr())
        bufs = {leg: (torch.zeros(n * cap1, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                      torch.zeros(n, dtype=torch.int32, device=dev)) for leg in LEGS}

        def once(leg):
            out, out_len, status = bufs[leg]
            if leg == "per_block":
                rc = lib.lz4flex_compress_batch_ex(ctx, p(src), p(in_off), p(in_len), None, n, p(out), p(out_off), p(out_cap), p(out_len),
                                                   p(status), C.byref(ext), L.MEM_DEVICE, sp)
            else:
                assert lib.lz4flex_set_tuning(ctx, b"compress_shared_dict", 1 if leg == "shared" else 0) == 0
                rc = lib.lz4flex_compress_batch_shared_dict(ctx, p(src), p(in_off), p(in_len), n, p(out), p(out_off), p(out_cap), p(out_len),
                                                            p(status), p(dic), dic.numel(), L.MEM_DEVICE, sp)
            assert rc == 0, (rc, L.last_error())

        times = {leg: [] for leg in LEGS}
        counted = None
        for r in range(args.warmup + args.reps):
            for leg in LEGS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                once(leg)
                e1.record(stream)
                e1.synchronize()
                if r >= args.warmup:
                    times[leg].append(e0.elapsed_time(e1))
                if leg == "shared" and counted is None:
                    counted = lib.lz4flex_get_tuning(ctx, b"debug_shared_dict_items")
        prof = {}
        if args.prof:
            lib.lz4flex_debug_wave_prof.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
            names = ["idx_busy", "idx_barrier", "match(sum of workers)", "wait_after_match", "place", "load_window", "wait_after_load"]
            for leg in LEGS:
                vals = (C.c_ulonglong * 32)()
                assert lib.lz4flex_debug_wave_prof(ctx, 1, None) == 0
                once(leg)
                torch.cuda.synchronize()
                assert lib.lz4flex_debug_wave_prof(ctx, 0, vals) == 0
                v = list(vals)
                nw = max(v[7], 1)
                prof[leg] = dict({nm: round(x / nw) for nm, x in zip(names, v)}, windows=v[7], supersteps_per_window=round(v[13] / nw, 2),
                                 encode_seqs_cycles_per_window=round(v[15] / nw))
        assert lib.lz4flex_set_tuning(ctx, b"compress_shared_dict", 1) == 0
        ref_out, ref_len, ref_st = bufs["per_block"]
        assert int((ref_st != 0).sum()) == 0, "compress status"
        same = {leg: bool(torch.equal(bufs[leg][1], ref_len)) and bool(torch.equal(bufs[leg][0], ref_out)) and int((bufs[leg][2] != 0).sum()) == 0
                for leg in LEGS}
        comp_total = int(ref_len.to(torch.int64).sum())
        out, out_len, _ = bufs["shared"]
        back = torch.empty(n * blk, dtype=torch.uint8, device=dev)
        b_len = torch.zeros(n, dtype=torch.int32, device=dev)
        b_st = torch.zeros(n, dtype=torch.int32, device=dev)
        dx = L.DecompressExt(dic.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), None, None, 0)
        rc = lib.lz4flex_decompress_batch_ex(ctx, p(out), p(out_off), p(out_len), n, p(back), p(in_off), p(in_len), p(b_len), p(b_st), None,
                                             C.byref(dx), L.MEM_DEVICE, sp)
        assert rc == 0, (rc, L.last_error())
        torch.cuda.synchronize()
        ok = int((b_st != 0).sum()) == 0 and bool((b_len == blk).all()) and bool(torch.equal(back, src))
        base = statistics.median(times["per_block"])
        for leg in LEGS:
            ms = statistics.median(times[leg])
            print(json.dumps({"workload": w, "what": what, "leg": leg, "ms": round(ms, 3), "ms_min": round(min(times[leg]), 3),
                              "ms_max": round(max(times[leg]), 3), "per_block_over_this": round(base / ms, 3),
                              "GiB_per_s": round(n * blk / 2**30 / (ms / 1e3), 2), "ratio": round(comp_total / (n * blk), 4),
                              "same_bytes_as_per_block": same[leg], "digest_items": counted if leg == "shared" else None,
                              "round_trip_ok": ok if leg == "shared" else None,
                              "cycles_per_window": prof.get(leg)}), flush=True)
        del src, bufs
        torch.cuda.empty_cache()
    lib.lz4flex_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
