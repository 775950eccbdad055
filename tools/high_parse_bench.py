#!/usr/bin/env python3
""""compress_parse" 0 (lazy) next to 1 (optimal) under compress_mode 2 ("high"), one session, the legs alternating: ms per
lz4flex_compress_batch call and ratio on the three device-resident shapes of tools/high_bench.py at depths 4, 16 and 64.  Every round
runs every leg once, in the same order; every block of every leg is decoded by the oracle's decoder (in the first round, outside the
timed part).  Not the reported bench (bench.py).  It needs torch only for the workload generators and the device buffers.

    python tools/high_parse_bench.py [--reps 3] [--scale 1.0] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WORKLOADS = (("16 384 x 64 KiB JSON tiles", "json", 16384, 65536), ("65 536 x 4 KiB log records", "log", 65536, 4096),
             ("256 x 4 MiB log blocks", "log", 256, 4 << 20))
LEGS = [(depth, parse) for depth in (4, 16, 64) for parse in (0, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of every workload's blocks")
    ap.add_argument("--out", help="append the lines to this file as well")
    args = ap.parse_args()
    import torch
    import oracle_api as O
    from lz4_flex_amd import _lib as L, workloads
    lib = L.load()
    dev = torch.device("cuda", 0)
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
    assert lib.lz4flex_set_tuning(ctx, b"compress_mode", 2) == 0
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sink = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

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
        mem = L.MEM_DEVICE | (L.MEM_BIG_BLOCKS if B > 65536 else 0)
        say("%s (%d blocks of %d bytes)" % (title, n, B))

        def once():
            assert lib.lz4flex_compress_batch(ctx, p(src), p(in_off), p(in_len), None, n, p(comp), p(comp_off), p(cap), p(clen), p(st), mem,
                                              stream) == 0, L.last_error()

        ms = {leg: [] for leg in LEGS}
        total = {}
        for rnd in range(args.reps + 1):            # round 0 warms up and is the one that is decoded
            for depth, parse in LEGS:
                assert lib.lz4flex_set_tuning(ctx, b"compress_depth", depth) == 0
                assert lib.lz4flex_set_tuning(ctx, b"compress_parse", parse) == 0
                e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                e[0].record(); once(); e[1].record()
                torch.cuda.synchronize()
                if rnd:
                    ms[(depth, parse)].append(e[0].elapsed_time(e[1]))
                    continue
                assert int((st != 0).sum().item()) == 0
                h_comp, h_len = comp.cpu().numpy(), clen.cpu().numpy()
                for k in range(n):
                    got = h_comp[k * stride:k * stride + int(h_len[k])].tobytes()
                    assert O.decompress(got, B) == ("ok", host[k * B:(k + 1) * B].tobytes()), (depth, parse, k)
                total[(depth, parse)] = int(h_len.sum())
        say("  %-24s %9s %9s %9s %8s %12s" % ("leg", "ms", "min", "max", "ratio", "bytes"))
        for depth, parse in LEGS:
            v = ms[(depth, parse)]
            say("  depth %-3d parse %d %-7s %9.1f %9.1f %9.1f %8.4f %12d" % (depth, parse, "optimal" if parse else "lazy", statistics.median(v),
                                                                         min(v), max(v), total[(depth, parse)] / (n * B), total[(depth, parse)]))
        for depth in (4, 16, 64):
            a, b = statistics.median(ms[(depth, 0)]), statistics.median(ms[(depth, 1)])
            say("  depth %-3d optimal / lazy: time %+.1f %% (%+.1f ms), bytes %+.2f %%" % (depth, 100.0 * (b / a - 1.0), b - a,
                                                                                        100.0 * (total[(depth, 1)] / total[(depth, 0)] - 1.0)))
        say("  every block of every leg decoded by the oracle")
    lib.lz4flex_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
