"""tools/dict_bench.py -- lz4flex_compress_batch_ex on device-resident batches: time (device events, after warm-up) and ratio of
compressing many blocks against one dictionary, in compress_mode fast (the throughput encoder) and exact (one-block chains of the
reference-exact chain encoder), next to fast without a dictionary.  Every output is decoded by lz4flex_decompress_batch_ex with the
dictionary and compared with the input on the device.

  (a) 16 384 x 64 KiB JSON tiles (workloads.json_tiles), one 32 KiB dictionary cut from JSON at another phase
  (b) 65 536 x 4 KiB log records (workloads.log_stream), one 32 KiB dictionary of other log lines

usage: python tools/dict_bench.py [--reps 5] [--warmup 2] [--workload a|b|both]   (one JSON line per leg)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import load_fixture  # noqa: E402
from lz4_flex_amd import _lib as L, block, workloads  # noqa: E402


def p(t):
    return C.c_void_p(t.data_ptr())


def workload(name, dev):
    if name == "a":
        plain = load_fixture(block, "compression_66k_JSON")
        n, blk = 16384, 65536
        src = workloads.json_tiles(plain, n * blk, phase=0, device=dev)
        dic = workloads.json_tiles(plain, 32768, phase=31337, device=dev)
        what = "16384 x 64 KiB JSON tiles, one 32 KiB JSON dictionary (another phase)"
    else:
        n, blk = 65536, 4096
        src = workloads.log_stream(0, n * blk, device=dev)
        dic = workloads.log_stream(workloads.LINE * 50_000_000, 32768, device=dev)
        what = "65536 x 4 KiB log records, one 32 KiB dictionary of other log lines"
    return what, src, dic, n, blk


def leg(lib, ctx, mode, use_dict, src, dic, n, blk, reps, warmup):
    dev = src.device
    assert lib.lz4flex_set_tuning(ctx, b"compress_mode", 1 if mode == "exact" else 0) == 0
    in_off = torch.arange(n, dtype=torch.int64, device=dev) * blk
    in_len = torch.full((n,), blk, dtype=torch.int32, device=dev)
    cap1 = 20 + blk * 110 // 100
    out = torch.empty(n * cap1, dtype=torch.uint8, device=dev)
    out_off = torch.arange(n, dtype=torch.int64, device=dev) * cap1
    out_cap = torch.full((n,), cap1, dtype=torch.int32, device=dev)
    out_len = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    d_off = torch.zeros(n, dtype=torch.int64, device=dev)
    d_len = torch.full((n,), dic.numel() if use_dict else 0, dtype=torch.int32, device=dev)
    ext = L.CompressExt(dic.data_ptr(), d_off.data_ptr(), d_len.data_ptr())
    stream = torch.cuda.current_stream(dev)

    def once():
        rc = lib.lz4flex_compress_batch_ex(ctx, p(src), p(in_off), p(in_len), None, n, p(out), p(out_off), p(out_cap), p(out_len), p(status),
                                           C.byref(ext) if use_dict else None, L.MEM_DEVICE, C.c_void_p(stream.cuda_stream))
        assert rc == 0, (rc, L.last_error())

    for _ in range(warmup):
        once()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        once()
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    assert int((status != 0).sum()) == 0, "compress status"
    comp_total = int(out_len.to(torch.int64).sum())
    # the round trip on the device: lz4flex_decompress_batch_ex with the dictionary
    back = torch.empty(n * blk, dtype=torch.uint8, device=dev)
    b_len = torch.zeros(n, dtype=torch.int32, device=dev)
    b_st = torch.zeros(n, dtype=torch.int32, device=dev)
    dx = L.DecompressExt(dic.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), None, None, 0)
    rc = lib.lz4flex_decompress_batch_ex(ctx, p(out), p(out_off), p(out_len), n, p(back), p(in_off), p(in_len), p(b_len), p(b_st), None,
                                         C.byref(dx) if use_dict else None, L.MEM_DEVICE, C.c_void_p(stream.cuda_stream))
    assert rc == 0, (rc, L.last_error())
    torch.cuda.synchronize()
    ok = int((b_st != 0).sum()) == 0 and bool((b_len == blk).all()) and bool(torch.equal(back, src))
    ms = statistics.median(times)
    return {"mode": mode, "dictionary": use_dict, "ms": round(ms, 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3),
            "GiB_per_s": round(n * blk / 2**30 / (ms / 1e3), 2), "ratio": round(comp_total / (n * blk), 4), "round_trip_ok": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", choices=["a", "b", "both"], default="both")
    args = ap.parse_args()
    lib = L.load()
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), -1) == 0
    dev = torch.device("cuda")
    for w in (["a", "b"] if args.workload == "both" else [args.workload]):
        what, src, dic, n, blk = workload(w, dev)
        for mode, use_dict in (("fast", True), ("exact", True), ("fast", False)):
            r = leg(lib, ctx, mode, use_dict, src, dic, n, blk, args.reps, args.warmup)
            print(json.dumps(dict({"workload": w, "what": what}, **r)), flush=True)
        del src
        torch.cuda.empty_cache()
    lib.lz4flex_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
