"""tools/packed_bench.py -- the packed batch entries next to the calls they wrap, on device-resident batches.  The legs ALTERNATE inside
one process; each round times one call of every leg with stream events, after --warmup rounds; median, minimum and maximum of --reps
rounds per leg, and every leg's output is compared with the input.

  shapes  (a) 16 384 x 64 KiB JSON tiles     (b) 65 536 x 4 KiB log records      (the workloads of tools/dict_bench.py, no dictionary)
  decode  plain          lz4flex_decompress_batch on slots the caller laid out (out_off = i * block size): the floor
          given          lz4flex_decompress_batch_packed, LZ4FLEX_SIZES_GIVEN       (the plain call + sizes, scan, finish)
          prepended      lz4flex_decompress_batch_packed, LZ4FLEX_SIZES_PREPENDED, on the stream the packed compress leg wrote
          scan           lz4flex_decompress_batch_packed, LZ4FLEX_SIZES_SCAN         (+ the size pass)
          scan_parent    block.decompress_blocks_device: size pass, torch.cumsum, a host synchronisation, an allocation, the plain call
  encode  plain_c        lz4flex_compress_batch into worst-case slots
          packed_c       lz4flex_compress_batch_packed, prepend_size = 1             (the plain call + sizes, two scans, the gather)
The layout kernels' own time is reported as the difference of the medians (given - plain: sizes + scan + finish; packed_c - plain_c:
sizes + two scans + gather): both sides are stream-event times of the same rounds.

usage: python tools/packed_bench.py [--reps 5] [--warmup 2] [--workload a|b|both]   (one JSON line per leg)"""
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
from lz4_flex_amd import block  # noqa: E402

LEGS = ("plain", "given", "prepended", "scan", "scan_parent", "plain_c", "packed_c")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", choices=["a", "b", "both"], default="both")
    args = ap.parse_args()
    lib = L.load()
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    for w in (["a", "b"] if args.workload == "both" else [args.workload]):
        what, src, dic, n, blk = workload(w, dev)
        del dic
        what = what.split(",")[0]
        i64 = lambda *a, **k: torch.zeros(*a, dtype=torch.int64, device=dev, **k)
        i32 = lambda *a, **k: torch.zeros(*a, dtype=torch.int32, device=dev, **k)
        in_off = torch.arange(n, dtype=torch.int64, device=dev) * blk
        in_len = torch.full((n,), blk, dtype=torch.int32, device=dev)
        cap1 = 20 + blk * 110 // 100
        c_off = torch.arange(n, dtype=torch.int64, device=dev) * cap1
        c_cap = torch.full((n,), cap1, dtype=torch.int32, device=dev)
        comp, c_len, c_st = torch.zeros(n * cap1, dtype=torch.uint8, device=dev), i32(n), i32(n)
        work = torch.empty(int(lib.lz4flex_packed_work_size(n)), dtype=torch.uint8, device=dev)
        scratch_cap = int(lib.lz4flex_compress_packed_scratch_bound(n * blk, n, 1))
        scratch = torch.empty(scratch_cap, dtype=torch.uint8, device=dev)
        stream_cap = n * blk // 2 + 8 * n
        packed, k_off, k_len, k_st = torch.zeros(stream_cap, dtype=torch.uint8, device=dev), i64(n + 1), i32(n), i32(n)
        out = {leg: torch.zeros(n * blk, dtype=torch.uint8, device=dev) for leg in ("plain", "given", "prepended", "scan")}
        res = {leg: (i64(n + 1), i32(n), i32(n), i32(n)) for leg in ("plain", "given", "prepended", "scan")}     # out_off, out_cap, out_len, status
        parent = {}

        def once(leg):
            if leg == "plain_c":
                rc = lib.lz4flex_compress_batch(None, p(src), p(in_off), p(in_len), None, n, p(comp), p(c_off), p(c_cap), p(c_len), p(c_st),
                                                L.MEM_DEVICE, sp)
            elif leg == "packed_c":
                rc = lib.lz4flex_compress_batch_packed(None, p(src), p(in_off), p(in_len), n, 1, p(scratch), scratch_cap, p(packed), stream_cap,
                                                       1, p(k_off), p(k_len), p(k_st), p(work), L.MEM_DEVICE, sp)
            elif leg == "plain":
                o_off, o_cap, o_len, o_st = res[leg]
                rc = lib.lz4flex_decompress_batch(None, p(comp), p(c_off), p(c_len), n, p(out[leg]), p(in_off), p(in_len), p(o_len), p(o_st), None,
                                                  L.MEM_DEVICE, sp)
            elif leg == "scan_parent":
                parent["r"] = block.decompress_blocks_device(comp, c_off, c_len)
                rc = 0
            else:
                o_off, o_cap, o_len, o_st = res[leg]
                mode = {"given": L.SIZES_GIVEN, "prepended": L.SIZES_PREPENDED, "scan": L.SIZES_SCAN}[leg]
                cb, co, cl = (packed, k_off, k_len) if leg == "prepended" else (comp, c_off, c_len)
                rc = lib.lz4flex_decompress_batch_packed(None, p(cb), p(co), p(cl), n, mode, p(in_len) if leg == "given" else None, p(out[leg]),
                                                         n * blk, 1, p(o_off), p(o_cap), p(o_len), p(o_st), None, p(work), L.MEM_DEVICE, sp)
            assert rc == 0, (leg, rc, L.last_error())

        order = ("plain_c", "packed_c", "plain", "given", "prepended", "scan", "scan_parent")      # (the encoders first: the decoders read their output)
        times = {leg: [] for leg in LEGS}
        for r in range(args.warmup + args.reps):
            for leg in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                once(leg)
                e1.record(stream)
                e1.synchronize()
                if r >= args.warmup:
                    times[leg].append(e0.elapsed_time(e1))
        torch.cuda.synchronize()
        ok = {leg: int((res[leg][3] != 0).sum()) == 0 and bool((res[leg][2] == blk).all()) and bool(torch.equal(out[leg], src))
              for leg in out}
        for leg in ("given", "prepended", "scan"):
            ok[leg] = ok[leg] and bool((res[leg][0][:n] == in_off).all()) and int(res[leg][0][n]) == n * blk
        ok["scan_parent"] = bool(torch.equal(parent["r"][0], src))
        ok["plain_c"] = int((c_st != 0).sum()) == 0
        k_end = int(k_off[n])
        ok["packed_c"] = int((k_st != 0).sum()) == 0 and bool((k_len == c_len + 4).all()) and k_end == int(c_len.to(torch.int64).sum()) + 4 * n
        med = {leg: statistics.median(times[leg]) for leg in LEGS}
        base = {"plain": "plain", "given": "plain", "prepended": "plain", "scan": "scan_parent", "scan_parent": "scan_parent",
                "plain_c": "plain_c", "packed_c": "plain_c"}
        for leg in LEGS:
            t = times[leg]
            print(json.dumps({"workload": w, "what": what, "leg": leg, "ms": round(med[leg], 3), "ms_min": round(min(t), 3),
                              "ms_max": round(max(t), 3), "spread_pct": round(100.0 * (max(t) - min(t)) / med[leg], 1),
                              "against": base[leg], "ms_over_it": round(med[leg] - med[base[leg]], 3),
                              "GiB_per_s": round(n * blk / 2**30 / (med[leg] / 1e3), 2),
                              "ratio": round(int(c_len.to(torch.int64).sum()) / (n * blk), 4), "output_ok": ok[leg]}), flush=True)
        del src, comp, packed, scratch, out, res, parent
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
