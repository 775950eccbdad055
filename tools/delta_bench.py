"""tools/delta_bench.py -- LZ4FLEX_FILTER_DELTA (the DELTA kernels of lz4_filter.hip) on device-resident data, the way tools/filter_bench.py
measures the plain filters and with its pieces: torch-free, the legs of a measurement ALTERNATE inside one session, each round times one
call of every leg with device events after --warmup rounds; median, minimum and maximum of --reps rounds per leg.  No time is a pass
condition.

  1. filters   per shape (16 384 x 64 KiB and 256 x 4 MiB: 1 GiB; 65 536 x 4 KiB: 256 MiB): a device-to-device copy of the same bytes, and
               every base filter (none, shuffle, bitshuffle) and its inverse per element size with and without the flag.  Every leg reads
               the shape's bytes once and writes them once; over_plain is a flagged leg's time over the same leg's without the flag.  The
               flagged legs' output is compared with the numpy model (tests/delta_filter_model.py) on the first and the last block, the
               inverse legs' with the input.
  2. codec     16 384 x 64 KiB of int64 timestamps (64 MiB of the generator, repeated): compressed / raw, compress time and decompress
               time of the typed entries with SHUFFLE, BITSHUFFLE and both with DELTA, E = 8, in compress_mode 0 (all blocks) and 2 (the
               first 1 024 blocks).

usage: python tools/delta_bench.py [--reps 5] [--warmup 2] [--only filters|codec] [--shapes 0,1,2] [--out profiles/r21_delta_filter.txt]
(one JSON line per leg)"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import delta_filter_model as DM  # noqa: E402
import filter_model as M  # noqa: E402
from dict_set_bench import Bench, Dev, hip, ok  # noqa: E402
from filter_bench import D2D, GIB, SHAPES, block_of, emit, stats  # noqa: E402
from lz4_flex_amd import _lib as L  # noqa: E402

NAMES = {M.NONE: "none", M.SHUFFLE: "shuffle", M.BITSHUFFLE: "bitshuffle"}


def leg_name(base, E, delta, inv):
    return "%s%s%s E=%d" % ("un" if inv else "", "delta+" if delta else "", NAMES[base], E)


def filters(B, sink, shapes):
    lib, ctx = B.lib, B.ctx
    piece = 64 << 20
    src = np.tile(np.random.default_rng(21).integers(0, 256, piece, dtype=np.uint8), GIB // piece)
    d_src, d_out, d_back = Dev(src), Dev(size=GIB), Dev(size=GIB)
    for s in shapes:
        n, blk = SHAPES[s]
        total = n * blk
        off, ln = Dev(np.arange(n, dtype=np.uint64) * blk), Dev(np.full(n, blk, np.uint32))

        def call(filt, E, inv, a, b):
            ok(lib.lz4flex_filter_batch(ctx, a.p, off.p, ln.p, n, b.p, off.p, filt, E, inv, L.MEM_DEVICE, None), "filter")

        # (FILTER_NONE without the flag is one kernel for every E)
        combos = [(f, E) for f in (M.NONE, M.SHUFFLE, M.BITSHUFFLE) for E in M.ELEMS]
        same = {}
        for f, E in combos:                              # forward into d_out, back into d_back: both checked before anything is timed
            call(f | L.FILTER_DELTA, E, 0, d_src, d_out)
            call(f | L.FILTER_DELTA, E, 1, d_out, d_back)
            ok(hip.hipDeviceSynchronize())
            same[(f, E)] = all((block_of(d_out, i, blk) == DM.forward(src[i * blk:(i + 1) * blk], f, E)).all() and
                               (block_of(d_back, i, blk) == src[i * blk:(i + 1) * blk]).all() for i in (0, n - 1))
        legs = {"copy": lambda: ok(hip.hipMemcpyAsync(d_out.p, d_src.p, total, D2D, None))}
        for f, E in combos:
            for delta in (0, 1):
                if f == M.NONE and not delta and E != 1:
                    continue
                filt = f | (L.FILTER_DELTA if delta else 0)
                legs[leg_name(f, E, delta, 0)] = lambda filt=filt, E=E: call(filt, E, 0, d_src, d_out)
                legs[leg_name(f, E, delta, 1)] = lambda filt=filt, E=E: call(filt, E, 1, d_src, d_back)
        dev, _wall = B.time(legs)
        copy_ms = statistics.median(dev["copy"])
        for f, E in combos:
            for inv in (0, 1):
                plain = leg_name(f, 1 if f == M.NONE else E, 0, inv)
                for delta in (0, 1):
                    k = leg_name(f, E, delta, inv)
                    if k not in dev:
                        continue
                    row = {"part": "filters", "shape": "%d x %d" % (n, blk), "mib": total >> 20, "leg": k}
                    row.update(stats(dev[k]))
                    row.update(gb_s=round(2.0 * total / 1e9 / (row["ms"] / 1e3), 1), over_copy=round(row["ms"] / copy_ms, 2))
                    if delta:
                        row.update(over_plain=round(row["ms"] / statistics.median(dev[plain]), 2), same_as_model=bool(same[(f, E)]))
                    emit(sink, row)
        row = {"part": "filters", "shape": "%d x %d" % (n, blk), "mib": total >> 20, "leg": "copy"}
        row.update(stats(dev["copy"]))
        row.update(gb_s=round(2.0 * total / 1e9 / (row["ms"] / 1e3), 1))
        emit(sink, row)
        off.free()
        ln.free()
    for d in (d_src, d_out, d_back):
        d.free()


def codec(B, sink):
    lib, ctx = B.lib, B.ctx
    n, blk = SHAPES[0]
    piece = 64 << 20
    E = 8
    cap1 = 20 + blk * 110 // 100
    off, ln = Dev(np.arange(n, dtype=np.uint64) * blk), Dev(np.full(n, blk, np.uint32))
    c_off, c_cap = Dev(np.arange(n, dtype=np.uint64) * cap1), Dev(np.full(n, cap1, np.uint32))
    d_tmp, d_back = Dev(size=GIB), Dev(size=GIB)
    src = np.tile(M.int64_timestamps(piece, 21), GIB // piece)
    d_src = Dev(src)
    kinds = {"shuffle": M.SHUFFLE, "bitshuffle": M.BITSHUFFLE, "delta+shuffle": M.SHUFFLE | L.FILTER_DELTA,
             "delta+bitshuffle": M.BITSHUFFLE | L.FILTER_DELTA}
    res = {k: (Dev(size=n * cap1), Dev(size=4 * n), Dev(size=4 * n)) for k in kinds}
    o_len, o_st = Dev(size=4 * n), Dev(size=4 * n)
    for mode, m in ((0, n), (2, 1024)):
        ok(lib.lz4flex_set_tuning(ctx, b"compress_mode", mode))

        def enc(k):
            out, ol, st = res[k]
            ok(lib.lz4flex_compress_batch_typed(ctx, d_src.p, off.p, ln.p, m, out.p, c_off.p, c_cap.p, ol.p, st.p, kinds[k], E, d_tmp.p, off.p,
                                                L.MEM_DEVICE, None), "compress " + k)

        def dec(k):
            out, ol, _st = res[k]
            ok(lib.lz4flex_decompress_batch_typed(ctx, out.p, c_off.p, ol.p, m, d_back.p, off.p, ln.p, o_len.p, o_st.p, None, kinds[k], E, d_tmp.p,
                                                  off.p, L.MEM_DEVICE, None), "decompress " + k)

        enc_ms, _wall = B.time({k: (lambda k=k: enc(k)) for k in kinds})
        ok(hip.hipDeviceSynchronize())
        ratio = {}
        for k in kinds:
            assert (res[k][2].get(np.int32)[:m] == 0).all()
            ratio[k] = round(float(res[k][1].get(np.uint32)[:m].sum(dtype=np.uint64)) / (m * blk), 4)
        same = {}
        for k in kinds:                                  # every leg gives the input back
            dec(k)
            ok(hip.hipDeviceSynchronize())
            same[k] = bool((o_st.get(np.int32)[:m] == 0).all() and all((block_of(d_back, i, blk) == src[i * blk:(i + 1) * blk]).all()
                                                                       for i in (0, m // 2, m - 1)))
        dec_ms, _wall = B.time({k: (lambda k=k: dec(k)) for k in kinds})
        for direction, ms in (("compress", enc_ms), ("decompress", dec_ms)):
            for k in kinds:
                row = {"part": "codec", "what": "int64 timestamps", "blocks": m, "compress_mode": mode, "filter": k, "E": E, "direction": direction}
                row.update(stats(ms[k]))
                row.update(gb_s=round(m * blk / 1e9 / (row["ms"] / 1e3), 1), ratio=ratio[k], right_bytes=same[k])
                emit(sink, row)
    ok(lib.lz4flex_set_tuning(ctx, b"compress_mode", 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--shapes", default="0,1,2")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sink = open(args.out, "a") if args.out else None
    lib = L.load()
    ctx = C.c_void_p()
    ok(lib.lz4flex_ctx_create(C.byref(ctx), -1), "ctx")
    B = Bench(lib, ctx, args.reps, args.warmup, sink)
    if args.only in ("", "filters"):
        filters(B, sink, [int(v) for v in args.shapes.split(",")])
    if args.only in ("", "codec"):
        codec(B, sink)
    lib.lz4flex_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
