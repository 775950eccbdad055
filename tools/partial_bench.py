#!/usr/bin/env python3
"""tools/partial_bench.py -- lz4flex_decompress_batch_partial next to a full decode of the same blocks, on device-resident batches of
64 KiB JSON tiles (the buffers are torch tensors, every codec call goes through ctypes as in tools/wave_bench.py).  The legs ALTERNATE
inside one session; each round times one call of every leg with device events, after --warmup rounds; the median, minimum and maximum
of --reps rounds are reported per leg, and every leg's output is compared with the input's first bytes.

  batches   4 096 and 16 384 blocks of 64 KiB
  targets   64, 4 096 and 65 536 bytes of every block
  legs      partial      lz4flex_decompress_batch_partial (the sequence decoder's partial form)
            partial_off  the entry with "decompress_partial" 0 (the reference's order, sixteen lanes per block, up to the target)
            full         lz4flex_decompress_batch of the whole blocks (what a caller without the entry has to do), default dispatch
            full_seq     the same pinned to the plain sequence decoder ("decompress_variant" 13): what a full-size target is expected to be level with

usage: python tools/partial_bench.py [--reps 7] [--warmup 2] [--blocks 4096 16384] [--targets 64 4096 65536]   (one JSON line per leg)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEGS = ("partial", "partial_off", "full", "full_seq")
B = 65536


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--blocks", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--targets", type=int, nargs="+", default=[64, 4096, 65536])
    args = ap.parse_args()
    import torch
    import oracle_api as O
    from lz4_flex_amd import _lib as L, workloads
    lib = L.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())     # noqa: E731
    ctxs = {}
    for leg, tuning in (("partial", {}), ("partial_off", {"decompress_partial": 0}), ("full", {}), ("full_seq", {"decompress_variant": 13})):
        ctxs[leg] = C.c_void_p()
        assert lib.lz4flex_ctx_create(C.byref(ctxs[leg]), 0) == 0
        for k, v in tuning.items():
            assert lib.lz4flex_set_tuning(ctxs[leg], k.encode(), v) == 0, k
    for n in args.blocks:
        src = workloads.json_tiles(O.fixture_plain("compression_66k_JSON"), n * B, device=dev)
        stride = (20 + B * 110 // 100 + 63) // 64 * 64
        comp = torch.empty(n * stride, dtype=torch.uint8, device=dev)
        ar = torch.arange(n, dtype=torch.int64, device=dev)
        in_off, comp_off = ar * B, ar * stride
        in_len = torch.full((n,), B, dtype=torch.int32, device=dev)
        cap = torch.full((n,), stride, dtype=torch.int32, device=dev)
        clen = torch.zeros(n, dtype=torch.int32, device=dev)
        st = torch.full((n,), -1, dtype=torch.int32, device=dev)
        assert lib.lz4flex_compress_batch(ctxs["full"], p(src), p(in_off), p(in_len), None, n, p(comp), p(comp_off), p(cap), p(clen), p(st),
                                          L.MEM_DEVICE, sp) == 0, L.last_error()
        torch.cuda.synchronize()
        assert int((st != 0).sum()) == 0, "compress status"
        for target in args.targets:
            t = min(target, B)
            want = {"full": B, "full_seq": B}
            back = {leg: (torch.zeros(n * want.get(leg, t), dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                          torch.full((n,), -1, dtype=torch.int32, device=dev)) for leg in LEGS}
            t_off = ar * t
            t_len = torch.full((n,), t, dtype=torch.int32, device=dev)

            def once(leg):
                out, out_len, bst = back[leg]
                if leg.startswith("full"):
                    rc = lib.lz4flex_decompress_batch(ctxs[leg], p(comp), p(comp_off), p(clen), n, p(out), p(in_off), p(in_len), p(out_len), p(bst),
                                                      None, L.MEM_DEVICE, sp)
                else:
                    rc = lib.lz4flex_decompress_batch_partial(ctxs[leg], p(comp), p(comp_off), p(clen), n, p(out), p(t_off), p(t_len), p(out_len),
                                                              p(bst), L.MEM_DEVICE, sp)
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
            torch.cuda.synchronize()
            first = src.view(n, B)[:, :t].contiguous().view(-1)
            base = statistics.median(times["full"])
            for leg in LEGS:
                out, out_len, bst = back[leg]
                size = want.get(leg, t)
                ok = int((bst != 0).sum()) == 0 and bool((out_len == size).all()) and bool(torch.equal(out, src if size == B else first))
                ms = statistics.median(times[leg])
                print(json.dumps({"blocks": n, "target": t, "leg": leg, "ms": round(ms, 3), "ms_min": round(min(times[leg]), 3),
                                  "ms_max": round(max(times[leg]), 3), "spread_pct": round(100.0 * (max(times[leg]) - min(times[leg])) / ms, 1),
                                  "full_over_this": round(base / ms, 3), "output_is_input": ok}), flush=True)
            del back
            torch.cuda.empty_cache()
        del src, comp
        torch.cuda.empty_cache()
    for c in ctxs.values():
        lib.lz4flex_ctx_destroy(c)


if __name__ == "__main__":
    main()
