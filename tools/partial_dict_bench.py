#!/usr/bin/env python3
"""tools/partial_dict_bench.py -- lz4flex_decompress_batch_partial_shared_dict / _dict_set next to a full decode of the same records, on
device-resident batches compressed by lz4flex_compress_batch_shared_dict against one 32 KiB dictionary (the buffers are torch tensors,
every codec call goes through ctypes as in tools/partial_bench.py).  The legs ALTERNATE inside one session; each round times one call
of every leg with device events, after --warmup rounds; the median, minimum and maximum of --reps rounds are reported per leg, and
every leg's output is compared with the input's first bytes.

  shapes    (b) 65 536 x 4 KiB log records     (a) 16 384 x 64 KiB JSON tiles      (the workloads of tools/dict_bench.py)
  targets   64, 512, 4 096 bytes of every block, and the block's full size
  legs      full         lz4flex_decompress_batch_shared_dict of the whole blocks (what a caller without the entry has to do)
            partial      lz4flex_decompress_batch_partial_shared_dict (the sequence decoder's form with a dictionary and a target)
            partial_off  the entry with "decompress_partial" 0 (the reference's order, sixteen lanes per block, up to the target)
            set4         target 512 only: lz4flex_decompress_batch_partial_dict_set, K = 4 (four copies of the dictionary, ids i mod 4)
  The one comparison to read off: `partial` at the full size against `full` of the same rounds -- "full_over_this" next to the spread of `full`.

usage: python tools/partial_dict_bench.py [--reps 7] [--warmup 2] [--workload a|b|both] [--targets 64 512 4096 0]   (0 = the full size; one JSON line per leg)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", choices=["a", "b", "both"], default="both")
    ap.add_argument("--targets", type=int, nargs="+", default=[64, 512, 4096, 0])
    args = ap.parse_args()
    import torch
    from dict_bench import p, workload
    from lz4_flex_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    ctx, off_ctx = C.c_void_p(), C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0 and lib.lz4flex_ctx_create(C.byref(off_ctx), 0) == 0
    assert lib.lz4flex_set_tuning(ctx, b"compress_mode", 0) == 0
    assert lib.lz4flex_set_tuning(off_ctx, b"decompress_partial", 0) == 0
    for w in (["b", "a"] if args.workload == "both" else [args.workload]):
        what, src, dic, n, blk = workload(w, dev)
        ar = torch.arange(n, dtype=torch.int64, device=dev)
        in_off = ar * blk
        in_len = torch.full((n,), blk, dtype=torch.int32, device=dev)
        cap1 = 20 + blk * 110 // 100
        c_off = ar * cap1
        c_cap = torch.full((n,), cap1, dtype=torch.int32, device=dev)
        comp = torch.zeros(n * cap1, dtype=torch.uint8, device=dev)
        clen = torch.zeros(n, dtype=torch.int32, device=dev)
        st = torch.full((n,), -1, dtype=torch.int32, device=dev)
        assert lib.lz4flex_compress_batch_shared_dict(ctx, p(src), p(in_off), p(in_len), n, p(comp), p(c_off), p(c_cap), p(clen), p(st), p(dic),
                                                      dic.numel(), L.MEM_DEVICE, sp) == 0, L.last_error()
        torch.cuda.synchronize()
        assert int((st != 0).sum()) == 0, "compress status"
        # K = 4: four copies of the dictionary in a set of their own memory
        four = dic.repeat(4).contiguous()
        k_off = torch.arange(4, dtype=torch.int64, device=dev) * dic.numel()
        k_len = torch.full((4,), dic.numel(), dtype=torch.int32, device=dev)
        dset = C.c_void_p()
        assert lib.lz4flex_dict_set_create(ctx, p(four), p(k_off), p(k_len), 4, L.MEM_DEVICE, C.byref(dset)) == 0, L.last_error()
        ids = (ar % 4).to(torch.int32).contiguous()
        for target in dict.fromkeys(min(t, blk) if t else blk for t in args.targets):
            t = target
            legs = ["full", "partial", "partial_off"] + (["set4"] if t == 512 else [])
            back = {leg: (torch.zeros(n * (blk if leg == "full" else t), dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                          torch.full((n,), -1, dtype=torch.int32, device=dev)) for leg in legs}
            t_off = ar * t
            t_len = torch.full((n,), t, dtype=torch.int32, device=dev)

            def once(leg):
                out, out_len, bst = back[leg]
                if leg == "full":
                    rc = lib.lz4flex_decompress_batch_shared_dict(ctx, p(comp), p(c_off), p(clen), n, p(out), p(in_off), p(in_len), p(out_len), p(bst),
                                                                  None, p(dic), dic.numel(), L.MEM_DEVICE, sp)
                elif leg == "set4":
                    rc = lib.lz4flex_decompress_batch_partial_dict_set(ctx, p(comp), p(c_off), p(clen), n, p(ids), p(out), p(t_off), p(t_len),
                                                                       p(out_len), p(bst), dset, L.MEM_DEVICE, sp)
                else:
                    rc = lib.lz4flex_decompress_batch_partial_shared_dict(ctx if leg == "partial" else off_ctx, p(comp), p(c_off), p(clen), n, p(out),
                                                                          p(t_off), p(t_len), p(out_len), p(bst), p(dic), dic.numel(), L.MEM_DEVICE, sp)
                assert rc == 0, (rc, L.last_error())

            times = {leg: [] for leg in legs}
            for r in range(args.warmup + args.reps):
                for leg in legs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    once(leg)
                    e1.record(stream)
                    e1.synchronize()
                    if r >= args.warmup:
                        times[leg].append(e0.elapsed_time(e1))
            torch.cuda.synchronize()
            first = src.view(n, blk)[:, :t].contiguous().view(-1)
            base = statistics.median(times["full"])
            for leg in legs:
                out, out_len, bst = back[leg]
                size = blk if leg == "full" else t
                ok = int((bst != 0).sum()) == 0 and bool((out_len == size).all()) and bool(torch.equal(out, src if size == blk else first))
                ms = statistics.median(times[leg])
                print(json.dumps({"workload": what, "blocks": n, "target": t, "leg": leg, "ms": round(ms, 3), "ms_min": round(min(times[leg]), 3),
                                  "ms_max": round(max(times[leg]), 3), "spread_pct": round(100.0 * (max(times[leg]) - min(times[leg])) / ms, 1),
                                  "full_over_this": round(base / ms, 3), "output_is_input": ok}), flush=True)
            del back
            torch.cuda.empty_cache()
        lib.lz4flex_dict_set_free(dset)
        del src, comp, four
        torch.cuda.empty_cache()
    lib.lz4flex_ctx_destroy(ctx)
    lib.lz4flex_ctx_destroy(off_ctx)


if __name__ == "__main__":
    main()
