"""tools/dict_train_bench.py -- lz4flex_dict_train on device-resident batches: the time of one MEM_DEVICE call and what the trained
dictionary is worth.  Torch-free: device memory, events and copies through the HIP runtime (ctypes).

Two workloads, each with a 32 KiB dictionary at segments 256, 512 and 2 048:
  log    65 536 x 4 KiB log-like records
  json   16 384 x 64 KiB JSON-like tiles
Per (workload, segment) one JSON line: device ms per call (events around one call, after --warmup calls; median, minimum and maximum of
--reps), the dictionary's length, and compressed / raw of lz4flex_compress_batch_shared_dict (compress_mode 0) over records that are NOT
among the samples (another seed of the same generator), against the trained dictionary, against the samples' first 32 KiB, and of
lz4flex_compress_batch without a dictionary.  --model adds the one-thread time of the scalar definition (tests/sim/dict_train_model.c)
on the same input and compares the bytes -- it needs no device when given with --no-gpu, and minutes per workload.
The shares of the count and score kernels come from a run of this tool under `rocprofv3 --kernel-trace --stats` with --reps 1
--warmup 0 --no-ratio.

The data is synthetic (numpy): `distinct` generated records repeated with a per-record stamp, as in tools/dict_set_bench.py.

usage: python tools/dict_train_bench.py [--workload log|json|all] [--segments 256,512,2048] [--reps 5] [--warmup 2] [--model] [--no-gpu]
                                        [--no-ratio] [--out profiles/r19_dict_train.txt]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dict_set_bench import json_bytes, log_bytes, tiled  # noqa: E402  (loads libamdhip64 as well)

DICT = 32768
WORKLOADS = {"log": ("65536 x 4 KiB log records", log_bytes, 65536, 4096, 2048, 4096),
             "json": ("16384 x 64 KiB JSON tiles", json_bytes, 16384, 65536, 64, 256)}     # name, generator, n, record, distinct, unseen


def unseen_records(gen, n, blk):
    return np.ascontiguousarray(gen(n * blk, 977))


def model_leg(src, n, blk, k):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dict_train_model as M
    M.lib()
    t0 = time.perf_counter()
    d, st = M.train_batch(src, np.arange(n, dtype=np.uint64) * blk, np.full(n, blk, np.uint32), DICT, k)
    return d, st, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all")
    ap.add_argument("--segments", default="256,512,2048")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--no-ratio", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sink = open(args.out, "a") if args.out else None
    segments = [int(v) for v in args.segments.split(",")]

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    if not args.no_gpu:
        import dict_set_bench as S
        from lz4_flex_amd import _lib as L
        hip, Dev, ok = S.hip, S.Dev, S.ok
        lib = L.load()
        ctx = C.c_void_p()
        ok(lib.lz4flex_ctx_create(C.byref(ctx), -1), "ctx")
        ok(lib.lz4flex_set_tuning(ctx, b"compress_mode", 0))
        e0, e1 = C.c_void_p(), C.c_void_p()
        ok(hip.hipEventCreate(C.byref(e0)))
        ok(hip.hipEventCreate(C.byref(e1)))

    for key in (WORKLOADS if args.workload == "all" else [args.workload]):
        what, gen, n, blk, distinct, n_unseen = WORKLOADS[key]
        src = tiled(gen, n, blk, distinct)
        if args.no_gpu:
            for k in segments:
                d, st, ms = model_leg(src, n, blk, k)
                emit({"workload": what, "segment": k, "model_one_thread_ms": round(ms, 1), "dict_len": len(d), "status": st})
            continue
        d_src = Dev(src)
        in_off, in_len = Dev(np.arange(n, dtype=np.uint64) * blk), Dev(np.full(n, blk, np.uint32))
        work = Dev(size=int(lib.lz4flex_dict_train_work_size(n)))
        d_dict, d_res = Dev(size=DICT), Dev(size=8)

        if not args.no_ratio:
            un = unseen_records(gen, n_unseen, blk)
            cap1 = 20 + blk * 110 // 100
            u_src = Dev(un)
            u_off, u_len = Dev(np.arange(n_unseen, dtype=np.uint64) * blk), Dev(np.full(n_unseen, blk, np.uint32))
            c_off, c_cap = Dev(np.arange(n_unseen, dtype=np.uint64) * cap1), Dev(np.full(n_unseen, cap1, np.uint32))
            c_out, c_len, c_st = Dev(size=n_unseen * cap1), Dev(size=4 * n_unseen), Dev(size=4 * n_unseen)
            piece = Dev(np.ascontiguousarray(src[:DICT]))

            def ratio(dictionary, length):
                if dictionary is None:
                    rc = lib.lz4flex_compress_batch(ctx, u_src.p, u_off.p, u_len.p, None, n_unseen, c_out.p, c_off.p, c_cap.p, c_len.p, c_st.p, L.MEM_DEVICE, None)
                else:
                    rc = lib.lz4flex_compress_batch_shared_dict(ctx, u_src.p, u_off.p, u_len.p, n_unseen, c_out.p, c_off.p, c_cap.p, c_len.p, c_st.p,
                                                                dictionary.p, length, L.MEM_DEVICE, None)
                ok(rc, "compress")
                ok(hip.hipDeviceSynchronize())
                assert (c_st.get(np.int32) == 0).all()
                return round(float(c_len.get(np.uint32).sum(dtype=np.uint64)) / un.size, 4)

            base = {"ratio_none": ratio(None, 0), "ratio_first_32k": ratio(piece, DICT)}

        for k in segments:
            def train():
                ok(lib.lz4flex_dict_train(ctx, d_src.p, in_off.p, in_len.p, n, d_dict.p, DICT, k, d_res.p, C.c_void_p(d_res.p.value + 4), work.p,
                                          L.MEM_DEVICE, None), "train")
            ms = []
            for r in range(args.warmup + args.reps):
                ok(hip.hipDeviceSynchronize())
                ok(hip.hipEventRecord(e0, None))
                train()
                ok(hip.hipEventRecord(e1, None))
                ok(hip.hipEventSynchronize(e1))
                v = C.c_float()
                ok(hip.hipEventElapsedTime(C.byref(v), e0, e1))
                if r >= args.warmup:
                    ms.append(v.value)
            dict_len, status = (int(x) for x in d_res.get(np.int32))
            m = statistics.median(ms)
            row = {"workload": what, "segment": k, "ms": round(m, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                   "scatter_pct": round(100.0 * (max(ms) - min(ms)) / m, 1), "dict_len": dict_len, "status": status}
            if not args.no_ratio:
                row.update(base, ratio_trained=ratio(d_dict, dict_len))
            if args.model:
                d, st, mms = model_leg(src, n, blk, k)
                row.update(model_one_thread_ms=round(mms, 1), same_bytes=bool(d == d_dict.get()[:dict_len].tobytes() and st == status))
            emit(row)
        ok(hip.hipDeviceSynchronize())
        for d in [d_src, in_off, in_len, work, d_dict, d_res] + ([] if args.no_ratio else [u_src, u_off, u_len, c_off, c_cap, c_out, c_len, c_st, piece]):
            d.free()
    if not args.no_gpu:
        lib.lz4flex_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
