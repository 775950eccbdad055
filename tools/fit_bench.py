"""tools/fit_bench.py -- the fit batches (lz4_fit.hip: lz4flex_fit_batch, lz4flex_compress_batch_fit) on device-resident data.  Torch-free:
device memory, events and copies through the HIP runtime (ctypes).  The legs of a measurement ALTERNATE inside one session; each round
times one call of every leg with device events after --warmup rounds; median, minimum and maximum of --reps rounds per leg.  No time is
a pass condition.

Per shape (65 536 x 4 KiB log records; 16 384 x 64 KiB JSON tiles) the blocks are compressed once (compress_mode 0) and every block is
then cut to the same capacity: 1/4, 1/2 and 1 x the batch's mean compressed size.  Legs per capacity:
  fit           lz4flex_fit_batch alone: walks at most cap bytes of every block, copies at most cap bytes
  size_scan     lz4flex_decompressed_size_batch on the same blocks: walks the WHOLE block, writes a size
  copy          a device-to-device copy of n x cap bytes (hipMemcpyAsync)
  compress      lz4flex_compress_batch into slots of the maximum output size
  compress_fit  lz4flex_compress_batch_fit: the same encoder into the scratch slots, the slot scan, the fit pass
"fit_over_scan_plus_copy" is fit / (size_scan + copy); the expectation it is held against is <= 1.10 at cap = 1/2.  The fit results are
checked first (status 0, out_len <= cap; a sample of blocks decoded by the model's rule is tests/test_gpu_fit.py's business, not this tool's).

usage: python tools/fit_bench.py [--reps 5] [--warmup 2] [--shapes 0,1] [--out profiles/r22_fit.txt]     (one JSON line per leg)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dict_set_bench import Bench, Dev, hip, json_bytes, log_bytes, ok, tiled  # noqa: E402  (loads libamdhip64 as well)
from lz4_flex_amd import _lib as L  # noqa: E402

hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
hip.hipMemcpyAsync.restype = C.c_int
D2D = 3
SHAPES = [("log records", log_bytes, 65536, 4096, 1024), ("JSON tiles", json_bytes, 16384, 65536, 256)]
FRACTIONS = [(1, 4), (1, 2), (1, 1)]


def emit(sink, row):
    line = json.dumps(row)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


def stats(ms):
    m = statistics.median(ms)
    return {"ms": round(m, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "scatter_pct": round(100.0 * (max(ms) - min(ms)) / m, 1)}


def shape(B, sink, what, gen, n, blk, distinct):
    lib, ctx = B.lib, B.ctx
    src = tiled(gen, n, blk, distinct)
    d_src = Dev(src)
    cap1 = 20 + blk * 110 // 100
    in_off, in_len = Dev(np.arange(n, dtype=np.uint64) * blk), Dev(np.full(n, blk, np.uint32))
    c_off, c_cap = Dev(np.arange(n, dtype=np.uint64) * cap1), Dev(np.full(n, cap1, np.uint32))
    comp, c_len, c_st = Dev(size=n * cap1), Dev(size=4 * n), Dev(size=4 * n)
    scratch_cap = int(lib.lz4flex_compress_packed_scratch_bound(n * blk, n, 0))
    scratch, work = Dev(size=scratch_cap), Dev(size=int(lib.lz4flex_compress_fit_work_size(n)))
    sizes, s_st = Dev(size=8 * n), Dev(size=4 * n)
    o_len, o_used, o_st = Dev(size=4 * n), Dev(size=4 * n), Dev(size=4 * n)

    def compress():
        ok(lib.lz4flex_compress_batch(ctx, d_src.p, in_off.p, in_len.p, None, n, comp.p, c_off.p, c_cap.p, c_len.p, c_st.p, L.MEM_DEVICE, None), "compress")

    ok(lib.lz4flex_set_tuning(ctx, b"compress_mode", 0))
    compress()
    ok(hip.hipDeviceSynchronize())
    assert (c_st.get(np.int32) == 0).all()
    lens = c_len.get(np.uint32)
    mean = float(lens.mean())
    for num, den in FRACTIONS:
        cap = int(mean * num / den)
        out, o_off, o_cap = Dev(size=n * cap), Dev(np.arange(n, dtype=np.uint64) * cap), Dev(np.full(n, cap, np.uint32))

        def fit():
            ok(lib.lz4flex_fit_batch(ctx, comp.p, c_off.p, c_len.p, d_src.p, in_off.p, in_len.p, n, out.p, o_off.p, o_cap.p, o_len.p, o_used.p,
                                     o_st.p, L.MEM_DEVICE, None), "fit")

        def scan():
            ok(lib.lz4flex_decompressed_size_batch(ctx, comp.p, c_off.p, c_len.p, n, None, sizes.p, s_st.p, L.MEM_DEVICE, None), "size scan")

        def compress_fit():
            ok(lib.lz4flex_compress_batch_fit(ctx, d_src.p, in_off.p, in_len.p, n, scratch.p, scratch_cap, out.p, o_off.p, o_cap.p, o_len.p,
                                              o_used.p, o_st.p, work.p, L.MEM_DEVICE, None), "compress_fit")

        results = {}
        for name, call in (("fit", fit), ("compress_fit", compress_fit)):      # both checked before anything is timed
            call()
            ok(hip.hipDeviceSynchronize())
            st, ln, used = o_st.get(np.int32), o_len.get(np.uint32), o_used.get(np.uint32)
            results[name] = {"all_ok": bool((st == 0).all() and (ln <= cap).all()), "fits_whole": int((used == blk).sum()),
                             "mean_used_fraction": round(float(used.mean()) / blk, 4), "mean_out_len": round(float(ln.mean()), 1)}
        same = results["fit"] == results["compress_fit"]
        legs = {"fit": fit, "size_scan": scan, "copy": lambda: ok(hip.hipMemcpyAsync(out.p, comp.p, n * cap, D2D, None)), "compress": compress,
                "compress_fit": compress_fit}
        dev, _wall = B.time(legs)
        med = {k: statistics.median(v) for k, v in dev.items()}
        for k, ms in dev.items():
            row = {"shape": "%d x %d %s" % (n, blk, what), "mean_compressed": round(mean, 1), "cap": cap, "cap_fraction": "%d/%d" % (num, den), "leg": k}
            row.update(stats(ms))
            if k == "fit":
                row.update(results["fit"], fit_over_scan_plus_copy=round(med["fit"] / (med["size_scan"] + med["copy"]), 3))
            if k == "compress_fit":
                row.update(results["compress_fit"], same_as_fit_leg=same, over_compress=round(med["compress_fit"] / med["compress"], 3))
            emit(sink, row)
        for d in (out, o_off, o_cap):
            d.free()
    for d in (d_src, in_off, in_len, c_off, c_cap, comp, c_len, c_st, scratch, work, sizes, s_st, o_len, o_used, o_st):
        d.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sink = open(args.out, "a") if args.out else None
    lib = L.load()
    ctx = C.c_void_p()
    ok(lib.lz4flex_ctx_create(C.byref(ctx), -1), "ctx")
    B = Bench(lib, ctx, args.reps, args.warmup, sink)
    for s in (int(v) for v in args.shapes.split(",")):
        shape(B, sink, *SHAPES[s])
    lib.lz4flex_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
