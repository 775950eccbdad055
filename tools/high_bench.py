#!/usr/bin/env python3
"""compress_mode 2 ("high") next to the other two encoders, one session: ms per lz4flex_compress_batch call and ratio on device-resident
batches, mode 2 at depths 4, 16 and 64; the CPU alternative (liblz4 LZ4_compress_HC at levels 3 and 9 on 16 host threads over the same
blocks); every GPU result is decoded by the oracle's decoder after the timing loop.  Not the reported bench (bench.py).  Like
wave_bench.py it needs torch only for the workload generators and the device buffers.

    python tools/high_bench.py [--reps 3] [--scale 1.0] [--no-cpu]
"""
import argparse
import concurrent.futures
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WORKLOADS = (("16 384 x 64 KiB JSON tiles", "json", 16384, 65536), ("65 536 x 4 KiB log records", "log", 65536, 4096),
             ("256 x 4 MiB log blocks", "log", 256, 4 << 20))
CONFIGS = (("mode 0 (fast)", 0, None), ("mode 1 (exact)", 1, None), ("mode 2, depth 4", 2, 4), ("mode 2, depth 16", 2, 16), ("mode 2, depth 64", 2, 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of every workload's blocks")
    ap.add_argument("--no-cpu", action="store_true", help="skip the liblz4 HC columns")
    args = ap.parse_args()
    import torch
    import oracle_api as O
    from lz4_flex_amd import _lib as L, workloads
    lib = L.load()
    dev = torch.device("cuda", 0)
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    hc = O.clz4()
    hc.LZ4_compress_HC.restype = C.c_int
    hc.LZ4_compress_HC.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    for title, data, n, B in WORKLOADS:
        n = max(1, int(n * args.scale))
        if data == "json":
            src = workloads.json_tiles(O.fixture_plain("compression_66k_JSON"), n * B, device=dev)
        else:
            src = workloads.log_stream(0, n * B, device=dev)
        stride = (20 + B * 110 // 100 + 63) // 64 * 64
        comp = torch.empty(n * stride, dtype=torch.uint8, device=dev)
        ar = torch.arange(n, dtype=torch.int64, device=dev)
        in_off, comp_off = ar * B, ar * stride
        in_len = torch.full((n,), B, dtype=torch.int32, device=dev)
        cap = torch.full((n,), stride, dtype=torch.int32, device=dev)
        clen = torch.zeros(n, dtype=torch.int32, device=dev)
        st = torch.full((n,), -1, dtype=torch.int32, device=dev)
        host = src.cpu().numpy()
        print("%s (%d blocks of %d bytes)" % (title, n, B), flush=True)
        for name, mode, depth in CONFIGS:
            assert lib.lz4flex_set_tuning(ctx, b"compress_mode", mode) == 0
            if depth:
                assert lib.lz4flex_set_tuning(ctx, b"compress_depth", depth) == 0

            def once():
                assert lib.lz4flex_compress_batch(ctx, p(src), p(in_off), p(in_len), None, n, p(comp), p(comp_off), p(cap), p(clen), p(st),
                                                  L.MEM_DEVICE | (L.MEM_BIG_BLOCKS if B > 65536 else 0), stream) == 0, L.last_error()

            once(); torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                e[0].record(); once(); e[1].record()
                torch.cuda.synchronize()
                ms.append(e[0].elapsed_time(e[1]))
            assert int((st != 0).sum().item()) == 0
            h_comp, h_len = comp.cpu().numpy(), clen.cpu().numpy()
            for k in range(n):
                got = h_comp[k * stride:k * stride + int(h_len[k])].tobytes()
                assert O.decompress(got, B) == ("ok", host[k * B:(k + 1) * B].tobytes()), (name, k)
            print("  %-18s ratio %.4f  ms per call %s  (every block decoded by the oracle)" % (name, float(h_len.sum()) / (n * B),
                                                                                       " ".join("%.2f" % x for x in ms)), flush=True)
        if args.no_cpu:
            continue
        bound = hc.LZ4_compressBound(B)
        for level in (3, 9):
            def work(lo, hi, level=level):
                out = C.create_string_buffer(bound)
                total = 0
                for k in range(lo, hi):
                    total += hc.LZ4_compress_HC(host.ctypes.data + k * B, out, B, bound, level)
                return total
            per = (n + 15) // 16
            t0 = time.perf_counter()
            with concurrent.futures.ThreadPoolExecutor(16) as ex:
                total = sum(ex.map(lambda i: work(min(i * per, n), min((i + 1) * per, n)), range(16)))
            print("  liblz4 HC level %d     ratio %.4f  ms, 16 host threads %.1f" % (level, total / (n * B), 1e3 * (time.perf_counter() - t0)), flush=True)
    lib.lz4flex_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
