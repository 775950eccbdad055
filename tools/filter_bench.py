"""tools/filter_bench.py -- the typed batches (lz4_filter.hip: lz4flex_filter_batch, lz4flex_compress_batch_typed,
lz4flex_decompress_batch_typed) on device-resident data.  Torch-free: device memory, events and copies through the HIP runtime
(ctypes).  The legs of a measurement ALTERNATE inside one session; each round times one call of every leg with device events after
--warmup rounds; median, minimum and maximum of --reps rounds per leg.  No time is a pass condition.

  1. filters   per shape (16 384 x 64 KiB and 256 x 4 MiB: 1 GiB; 65 536 x 4 KiB: 256 MiB): a device-to-device copy of the same bytes
               (hipMemcpyAsync), each filter and its inverse per element size, and the same under "filter_bytewise" 1 (the narrow
               path).  Every leg reads the shape's bytes once and writes them once; gb_s is that traffic over the time.  The forward
               legs' output is compared with the numpy model (tests/filter_model.py) on the first and the last block, the inverse
               legs' with the input.
  2. codec     16 384 x 64 KiB of bf16 N(0, 0.02) weights (bitshuffle, E = 2) and of int64 timestamps (shuffle, E = 8): the typed
               entries against the plain ones in compress_mode 0, both directions -- and against the plain entries over the filtered
               bytes, which is the typed call without its filter pass -- and compressed / raw with and without the filter in
               compress_mode 0 and 2 (mode 2 over the first 1 024 blocks).  The data is 64 MiB of the generator, repeated.

usage: python tools/filter_bench.py [--reps 5] [--warmup 2] [--only filters|codec] [--shapes 0,1,2] [--no-bytewise] [--out profiles/r20_filters.txt]
(one JSON line per leg)"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import filter_model as M  # noqa: E402
from dict_set_bench import Bench, Dev, hip, ok  # noqa: E402  (loads libamdhip64 as well)
from lz4_flex_amd import _lib as L  # noqa: E402

hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
hip.hipMemcpyAsync.restype = C.c_int
D2D = 3
GIB = 1 << 30
SHAPES = [(16384, 65536), (65536, 4096), (256, 4 << 20)]
NAMES = {M.SHUFFLE: "shuffle", M.BITSHUFFLE: "bitshuffle"}


def emit(sink, row):
    line = json.dumps(row)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


def stats(ms):
    m = statistics.median(ms)
    return {"ms": round(m, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "scatter_pct": round(100.0 * (max(ms) - min(ms)) / m, 1)}


def block_of(dev, i, blk):
    out = np.empty(blk, np.uint8)
    ok(hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(dev.p.value + i * blk), blk, 2))
    return out


def filters(B, sink, shapes, bytewise):
    lib, ctx = B.lib, B.ctx
    src = np.random.default_rng(20).integers(0, 256, GIB, dtype=np.uint8)
    d_src, d_out, d_back = Dev(src), Dev(size=GIB), Dev(size=GIB)
    for s in shapes:
        n, blk = SHAPES[s]
        total = n * blk                                  # (65 536 x 4 KiB is 256 MiB: the front of the buffers)
        off, ln = Dev(np.arange(n, dtype=np.uint64) * blk), Dev(np.full(n, blk, np.uint32))

        def call(filt, E, inv, a, b):
            ok(lib.lz4flex_filter_batch(ctx, a.p, off.p, ln.p, n, b.p, off.p, filt, E, inv, L.MEM_DEVICE, None), "filter")

        combos = [(f, E) for f in (M.SHUFFLE, M.BITSHUFFLE) for E in M.ELEMS]
        for wide in ([1, 0] if bytewise else [1]):
            ok(lib.lz4flex_set_tuning(ctx, b"filter_bytewise", 0 if wide else 1))
            same = {}
            for f, E in combos:                          # forward into d_out, back into d_back: both checked before anything is timed
                call(f, E, 0, d_src, d_out)
                call(f, E, 1, d_out, d_back)
                ok(hip.hipDeviceSynchronize())
                same[(f, E)] = all((block_of(d_out, i, blk) == M.forward(src[i * blk:(i + 1) * blk], f, E)).all() and
                                   (block_of(d_back, i, blk) == src[i * blk:(i + 1) * blk]).all() for i in (0, n - 1))
            legs = {"copy": lambda: ok(hip.hipMemcpyAsync(d_out.p, d_src.p, total, D2D, None))}
            for f, E in combos:
                legs["%s E=%d" % (NAMES[f], E)] = lambda f=f, E=E: call(f, E, 0, d_src, d_out)
                legs["un%s E=%d" % (NAMES[f], E)] = lambda f=f, E=E: call(f, E, 1, d_src, d_back)
            dev, _wall = B.time(legs)
            copy_ms = statistics.median(dev["copy"])
            for k, ms in dev.items():
                row = {"part": "filters", "shape": "%d x %d" % (n, blk), "mib": total >> 20, "path": "wide" if wide else "bytewise", "leg": k}
                row.update(stats(ms))
                row.update(gb_s=round(2.0 * total / 1e9 / (row["ms"] / 1e3), 1), over_copy=round(row["ms"] / copy_ms, 2))
                if k != "copy":
                    f = M.BITSHUFFLE if "bitshuffle" in k else M.SHUFFLE
                    row["same_as_model"] = bool(same[(f, int(k[-1]))])
                emit(sink, row)
        ok(lib.lz4flex_set_tuning(ctx, b"filter_bytewise", 0))
        off.free()
        ln.free()
    for d in (d_src, d_out, d_back):
        d.free()


def codec(B, sink):
    lib, ctx = B.lib, B.ctx
    n, blk = SHAPES[0]
    piece = 64 << 20
    cap1 = 20 + blk * 110 // 100
    off, ln = Dev(np.arange(n, dtype=np.uint64) * blk), Dev(np.full(n, blk, np.uint32))
    c_off, c_cap = Dev(np.arange(n, dtype=np.uint64) * cap1), Dev(np.full(n, cap1, np.uint32))
    d_tmp, d_back = Dev(size=GIB), Dev(size=GIB)
    # plain: the plain entries on the raw data; typed: the typed entries; codec_alone: the plain entries on the FILTERED bytes (the tmp
    # slots of the last typed call; decode: the typed call's blocks into the slots) -- what the typed call costs without its filter pass
    res = {k: (Dev(size=n * cap1), Dev(size=4 * n), Dev(size=4 * n)) for k in ("plain", "typed", "codec_alone")}
    o_len, o_st = Dev(size=4 * n), Dev(size=4 * n)
    for what, data, filt, E in (("bf16 N(0, 0.02)", M.bf16_weights(piece, 20), M.BITSHUFFLE, 2),
                                ("int64 timestamps", M.int64_timestamps(piece, 21), M.SHUFFLE, 8)):
        src = np.tile(data, GIB // piece)
        d_src = Dev(src)

        def enc(k, m=n):
            out, ol, st = res[k]
            if k != "typed":
                rc = lib.lz4flex_compress_batch(ctx, (d_src if k == "plain" else d_tmp).p, off.p, ln.p, None, m, out.p, c_off.p, c_cap.p, ol.p, st.p,
                                                L.MEM_DEVICE, None)
            else:
                rc = lib.lz4flex_compress_batch_typed(ctx, d_src.p, off.p, ln.p, m, out.p, c_off.p, c_cap.p, ol.p, st.p, filt, E, d_tmp.p, off.p,
                                                      L.MEM_DEVICE, None)
            ok(rc, "compress " + k)

        def dec(k):
            out, ol, _st = res[k]
            if k != "typed":
                rc = lib.lz4flex_decompress_batch(ctx, out.p, c_off.p, ol.p, n, (d_back if k == "plain" else d_tmp).p, off.p, ln.p, o_len.p, o_st.p, None,
                                                  L.MEM_DEVICE, None)
            else:
                rc = lib.lz4flex_decompress_batch_typed(ctx, out.p, c_off.p, ol.p, n, d_back.p, off.p, ln.p, o_len.p, o_st.p, None, filt, E, d_tmp.p,
                                                        off.p, L.MEM_DEVICE, None)
            ok(rc, "decompress " + k)

        def ratio(k, m):
            ok(hip.hipDeviceSynchronize())
            assert (res[k][2].get(np.int32)[:m] == 0).all()
            return round(float(res[k][1].get(np.uint32)[:m].sum(dtype=np.uint64)) / (m * blk), 4)

        ok(lib.lz4flex_set_tuning(ctx, b"compress_mode", 2))
        m2 = 1024
        for k in res:
            enc(k, m2)
        high = {k: ratio(k, m2) for k in res}
        ok(lib.lz4flex_set_tuning(ctx, b"compress_mode", 0))
        dev, _wall = B.time({k: (lambda k=k: enc(k)) for k in res})
        fast = {k: ratio(k, n) for k in res}
        for k in res:
            row = {"part": "codec", "what": what, "filter": NAMES[filt], "E": E, "direction": "compress", "leg": k}
            row.update(stats(dev[k]))
            row.update(gb_s_in=round(GIB / 1e9 / (row["ms"] / 1e3), 1), ratio_mode0=fast[k], ratio_mode2_first_1024=high[k])
            emit(sink, row)
        same = {}
        for k in res:                                    # every leg gives the input back
            dec(k)
            ok(hip.hipDeviceSynchronize())
            want = (lambda b: M.forward(b, filt, E)) if k == "codec_alone" else (lambda b: b)      # (that leg decodes to the filtered bytes)
            same[k] = bool((o_st.get(np.int32) == 0).all() and all((block_of(d_tmp if k == "codec_alone" else d_back, i, blk) ==
                                                                    want(src[i * blk:(i + 1) * blk])).all() for i in (0, n // 2, n - 1)))
        dev, _wall = B.time({k: (lambda k=k: dec(k)) for k in res})
        for k in res:
            row = {"part": "codec", "what": what, "filter": NAMES[filt], "E": E, "direction": "decompress", "leg": k}
            row.update(stats(dev[k]))
            row.update(gb_s_out=round(GIB / 1e9 / (row["ms"] / 1e3), 1), right_bytes=same[k])
            emit(sink, row)
        d_src.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--shapes", default="0,1,2")
    ap.add_argument("--no-bytewise", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sink = open(args.out, "a") if args.out else None
    lib = L.load()
    ctx = C.c_void_p()
    ok(lib.lz4flex_ctx_create(C.byref(ctx), -1), "ctx")
    B = Bench(lib, ctx, args.reps, args.warmup, sink)
    if args.only in ("", "filters"):
        filters(B, sink, [int(v) for v in args.shapes.split(",")], not args.no_bytewise)
    if args.only in ("", "codec"):
        codec(B, sink)
    lib.lz4flex_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
