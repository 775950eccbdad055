#!/usr/bin/env python3
"""Time of the decompressed-size query (lz4flex_decompressed_size_batch, lz4_size_scan.hip) next to the decode of the same batch
(lz4flex_decompress_batch, default dispatch), both DEVICE batches on one stream, event-timed; the sizes are checked against the plain
lengths.  Not the reported bench (bench.py).  Kernel times: run it under `rocprofv3 --kernel-trace --stats` (profiles/r07_size_scan.txt).

  python tools/size_scan_bench.py                     # the default shapes
  python tools/size_scan_bench.py --shapes json:65536:16384 --reps 20
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEFAULT = "json:65536:16384,json:65536:4096,text:65536:4096,random:65536:16384,log:4194304:256,log:16777216:1"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    import oracle_api as O
    from lz4_flex_amd import _lib as L, workloads
    lib = L.load()
    dev = torch.device("cuda", 0)
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    print("%-8s %9s %6s %10s %10s %10s %8s" % ("data", "block", "n", "GiB", "scan ms", "decode ms", "scan/dec"))
    for shape in args.shapes.split(","):
        data, B, n = shape.split(":")
        B, n = int(B), int(n)
        if data == "json":
            src = workloads.json_tiles(O.fixture_plain("compression_66k_JSON"), n * B, device=dev)
        elif data == "text":
            src = workloads.json_tiles(O.fixture_plain("compression_65k"), n * B, device=dev)
        elif data == "log":
            src = workloads.log_stream(0, n * B, device=dev)
        else:
            src = torch.randint(0, 256, (n * B,), dtype=torch.uint8, device=dev)
        big = L.MEM_BIG_BLOCKS if B > 65536 else 0
        stride = (20 + B * 110 // 100 + 63) // 64 * 64
        comp = torch.empty(n * stride, dtype=torch.uint8, device=dev)
        back = torch.empty(n * B, dtype=torch.uint8, device=dev)
        ar = torch.arange(n, dtype=torch.int64, device=dev)
        in_off, comp_off = ar * B, ar * stride
        in_len = torch.full((n,), B, dtype=torch.int32, device=dev)
        cap = torch.full((n,), stride, dtype=torch.int32, device=dev)
        comp_len = torch.zeros(n, dtype=torch.int32, device=dev)
        st = torch.zeros(n, dtype=torch.int32, device=dev)
        assert lib.lz4flex_compress_batch(ctx, p(src), p(in_off), p(in_len), None, n, p(comp), p(comp_off), p(cap), p(comp_len), p(st),
                                          L.MEM_DEVICE | big, stream) == 0
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0
        size = torch.zeros(n, dtype=torch.int64, device=dev)
        sst = torch.zeros(n, dtype=torch.int32, device=dev)
        out_len = torch.zeros(n, dtype=torch.int32, device=dev)
        dst = torch.zeros(n, dtype=torch.int32, device=dev)

        def scan():
            assert lib.lz4flex_decompressed_size_batch(ctx, p(comp), p(comp_off), p(comp_len), n, None, p(size), p(sst), L.MEM_DEVICE | big,
                                                       stream) == 0

        def decode():
            assert lib.lz4flex_decompress_batch(ctx, p(comp), p(comp_off), p(comp_len), n, p(back), p(in_off), p(in_len), p(out_len), p(dst),
                                                None, L.MEM_DEVICE | big, stream) == 0

        def timed(fn):
            fn()
            torch.cuda.synchronize()
            best = None
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                t = e0.elapsed_time(e1)
                best = t if best is None else min(best, t)
            return best

        ts = timed(scan)
        td = timed(decode)
        assert int(sst.abs().sum()) == 0 and bool((size == B).all()), "size scan disagrees with the plain lengths"
        assert int(dst.abs().sum()) == 0 and torch.equal(back, src)
        print("%-8s %9d %6d %10.3f %10.3f %10.3f %8.2f" % (data, B, n, n * B / 2 ** 30, ts, td, ts / td), flush=True)
        del src, comp, back
        torch.cuda.empty_cache()
    lib.lz4flex_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
