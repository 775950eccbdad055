#!/usr/bin/env python3
"""Wall time of every MEM_HOST path of the C ABI (capi.cpp, lz4_host_stage.h) at a user's size: --blocks blocks of --block-bytes log
bytes through pageable host memory, and the 1-block scalar calls.  A host clock around calls that return after their last
synchronisation.  Not the reported bench (bench.py).  LZ4FLEX_LIB=<path> times another build of the library.

  python tools/host_stage_bench.py                    # 1 024 x 64 KiB, 7 timed calls per line after 2 warm-up calls
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--block-bytes", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    from lz4_flex_amd import _lib as L, workloads
    lib = L.load()
    n, B = args.blocks, args.block_bytes
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0, L.last_error()
    p = lambda a: C.c_void_p(a.ctypes.data)
    u32, u64 = (lambda v: np.full(n, v, np.uint32)), (lambda step: np.arange(n, dtype=np.uint64) * np.uint64(step))

    plain = workloads.log_stream(0, n * B).numpy().copy()
    slot = int(lib.lz4flex_get_maximum_output_size(B))
    in_off, in_len, slot_off, slot_cap = u64(B), u32(B), u64(slot), u32(slot)
    comp, comp2, back = np.zeros(n * slot + 64, np.uint8), np.zeros(n * slot + 64, np.uint8), np.zeros(n * B + 64, np.uint8)
    out_len, status, used, detail = u32(0), np.zeros(n, np.int32), u32(0), np.zeros(2 * n, np.uint64)
    size, res_off = np.zeros(n, np.uint64), np.zeros(n + 1, np.uint64)
    HOST = L.MEM_HOST

    def ok(rc, st=status):
        assert rc == 0 and not st.any(), (rc, L.last_error(), st[:8])

    def must(v):
        assert v, L.last_error()

    # the compressed blocks every decode line and the fit line read: the library's own, in their slots (the compress lines write comp2)
    ok(lib.lz4flex_compress_batch(ctx, p(plain), p(in_off), p(in_len), None, n, p(comp), p(slot_off), p(slot_cap), p(out_len), p(status), HOST, None))
    c_len = out_len.copy()
    half = np.maximum(c_len // 2, 1).astype(np.uint32)
    bound = int(lib.lz4flex_compress_packed_scratch_bound(n * B, n, 0))
    one_len, dict_len, dict_st, dic = int(c_len[0]), np.zeros(1, np.uint32), np.zeros(1, np.int32), np.zeros(65536, np.uint8)

    lines = [
        ("compress_into, 1 block", lambda: must(lib.lz4flex_compress_into(p(plain), B, p(comp2), slot) > 0)),
        ("decompress_into, 1 block", lambda: must(lib.lz4flex_decompress_into(p(comp), one_len, p(back), B, None) == B)),
        ("compress_batch", lambda: ok(lib.lz4flex_compress_batch(ctx, p(plain), p(in_off), p(in_len), None, n, p(comp2), p(slot_off), p(slot_cap), p(out_len),
                                                              p(status), HOST, None))),
        ("decompress_batch", lambda: ok(lib.lz4flex_decompress_batch(ctx, p(comp), p(slot_off), p(c_len), n, p(back), p(in_off), p(in_len), p(out_len),
                                                                  p(status), p(detail), HOST, None))),
        ("decompressed_size_batch", lambda: ok(lib.lz4flex_decompressed_size_batch(ctx, p(comp), p(slot_off), p(c_len), n, None, p(size), p(status), HOST, None))),
        ("decompress_batch_packed", lambda: ok(lib.lz4flex_decompress_batch_packed(ctx, p(comp), p(slot_off), p(c_len), n, L.SIZES_GIVEN, p(in_len), p(back), n * B,
                                                                                16, p(res_off), p(used), p(out_len), p(status), p(detail), None, HOST, None))),
        ("compress_batch_packed", lambda: ok(lib.lz4flex_compress_batch_packed(ctx, p(plain), p(in_off), p(in_len), n, 0, None, bound, p(comp2), n * slot, 16,
                                                                            p(res_off), p(out_len), p(status), None, HOST, None))),
        ("dict_train", lambda: ok(lib.lz4flex_dict_train(ctx, p(plain), p(in_off), p(in_len), n, p(dic), 65536, 0, p(dict_len), p(dict_st), None, HOST, None), dict_st)),
        ("compress_batch_typed", lambda: ok(lib.lz4flex_compress_batch_typed(ctx, p(plain), p(in_off), p(in_len), n, p(comp2), p(slot_off), p(slot_cap), p(out_len),
                                                                          p(status), L.FILTER_SHUFFLE, 4, None, None, HOST, None))),
        ("fit_batch", lambda: ok(lib.lz4flex_fit_batch(ctx, p(comp), p(slot_off), p(c_len), p(plain), p(in_off), p(in_len), n, p(back), p(in_off), p(half),
                                                    p(out_len), p(used), p(status), HOST, None))),
        ("compress_batch_fit", lambda: ok(lib.lz4flex_compress_batch_fit(ctx, p(plain), p(in_off), p(in_len), n, None, 0, p(back), p(in_off), p(half), p(out_len),
                                                                      p(used), p(status), None, HOST, None))),
    ]
    result = {}
    for name, call in lines:
        for _ in range(args.warmup):
            call()
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        ms.sort()
        result[name] = ms[len(ms) // 2]
        print("%-28s median %9.3f ms   (%9.3f - %9.3f)" % (name, ms[len(ms) // 2], ms[0], ms[-1]))
    lib.lz4flex_ctx_destroy(ctx)
    print(json.dumps({"host_stage_bench_ms": result, "blocks": n, "block_bytes": B, "build_id": lib.lz4flex_build_id().decode()}))


if __name__ == "__main__":
    main()
