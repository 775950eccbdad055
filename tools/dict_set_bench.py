"""tools/dict_set_bench.py -- dictionary sets (lz4flex_dict_set_*, lz4flex_*_batch_dict_set) next to the entries they are defined by, both
directions, on device-resident batches.  Torch-free: device memory, events and copies through the HIP runtime (ctypes).  The legs of a
measurement ALTERNATE inside one session; each round times one call of every leg with device events after --warmup rounds; median,
minimum and maximum of --reps rounds per leg; every leg's output is compared with the first leg's (compress: the bytes; decompress: the
input).

  1. K = 1, large batches   set against lz4flex_*_batch_shared_dict: 65 536 x 4 KiB log-like records, 16 384 x 64 KiB JSON-like tiles
  2. K = 1, small batches   256 and 1 024 x 4 KiB records per call, repeated calls: what the prepared digest saves per call (the shared entry
                            runs its digest kernel in front of every launch), device events and host wall clock per call
  3. K = 4, interleaved     65 536 x 4 KiB records, ids cycling, against lz4flex_*_batch_ex with per-block dictionary arrays

The data is synthetic (numpy): records of a log-like line grammar and tiles of a JSON-like one, the dictionaries earlier output of the
same generators -- the legs are compared with each other on the same bytes, not with other tools' figures.

usage: python tools/dict_set_bench.py [--reps 5] [--warmup 2] [--only 1|2|3] [--out profiles/r12_dict_set.txt]   (one JSON line per leg)"""
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

from lz4_flex_amd import _lib as L  # noqa: E402

hip = C.CDLL("libamdhip64.so")
for name, args in (("hipMalloc", [C.POINTER(C.c_void_p), C.c_size_t]), ("hipFree", [C.c_void_p]),
                   ("hipMemcpy", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]), ("hipMemset", [C.c_void_p, C.c_int, C.c_size_t]),
                   ("hipDeviceSynchronize", []), ("hipEventCreate", [C.POINTER(C.c_void_p)]), ("hipEventRecord", [C.c_void_p, C.c_void_p]),
                   ("hipEventSynchronize", [C.c_void_p]), ("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p])):
    getattr(hip, name).argtypes = args
    getattr(hip, name).restype = C.c_int
H2D, D2H = 1, 2


def ok(rc, what="hip"):
    assert rc == 0, (what, rc, L.last_error())


class Dev:
    """a device buffer that holds a numpy array's bytes (or `size` zero bytes)"""

    def __init__(self, a=None, size=0):
        self.n = int(a.nbytes) if a is not None else int(size)
        self.p = C.c_void_p()
        ok(hip.hipMalloc(C.byref(self.p), max(self.n, 1)))
        if a is not None:
            a = np.ascontiguousarray(a)
            ok(hip.hipMemcpy(self.p, C.c_void_p(a.ctypes.data), self.n, H2D))
        else:
            ok(hip.hipMemset(self.p, 0, max(self.n, 1)))

    def get(self, dtype=np.uint8):
        out = np.empty(self.n // np.dtype(dtype).itemsize, dtype)
        ok(hip.hipMemcpy(C.c_void_p(out.ctypes.data), self.p, self.n, D2H))
        return out

    def free(self):
        if self.p:
            hip.hipFree(self.p)
        self.p = C.c_void_p()


def log_bytes(n, seed):
    rng = np.random.default_rng(seed)
    lvl, svc = [b"INFO ", b"WARN ", b"DEBUG", b"ERROR"], [b"auth", b"billing", b"search", b"ingest", b"gateway"]
    msg = [b"request completed", b"cache miss for key", b"retrying upstream call", b"connection reset by peer", b"user session refreshed"]
    out, size, t = [], 0, 1700000000
    while size < n:
        t += int(rng.integers(0, 3))
        line = b"%d.%03d %s svc=%s host=node-%02d req=%08x dur_ms=%d msg=\"%s\"\n" % (
            t, rng.integers(0, 1000), lvl[rng.integers(0, 4)], svc[rng.integers(0, 5)], rng.integers(0, 40), rng.integers(0, 1 << 32),
            rng.integers(1, 900), msg[rng.integers(0, 5)])
        out.append(line)
        size += len(line)
    return np.frombuffer(b"".join(out)[:n], np.uint8)


def json_bytes(n, seed):
    rng = np.random.default_rng(seed)
    tags = [b"alpha", b"beta", b"gamma", b"delta", b"epsilon", b"zeta"]
    out, size, i = [], 0, int(rng.integers(0, 1 << 20))
    while size < n:
        i += 1
        rec = b'{"id":%d,"type":"Feature","properties":{"name":"item-%d","score":%d.%02d,"tags":["%s","%s"],"active":%s},"geometry":{"type":"Point","coordinates":[%d.%05d,%d.%05d]}},\n' % (
            i, rng.integers(0, 100000), rng.integers(0, 100), rng.integers(0, 100), tags[rng.integers(0, 6)], tags[rng.integers(0, 6)],
            b"true" if rng.integers(0, 2) else b"false", rng.integers(-180, 180), rng.integers(0, 100000), rng.integers(-90, 90), rng.integers(0, 100000))
        out.append(rec)
        size += len(rec)
    return np.frombuffer(b"".join(out)[:n], np.uint8)


def tiled(gen, n, blk, distinct):
    """n blocks of blk bytes: `distinct` generated ones, repeated with a per-block stamp so that no two blocks are equal"""
    base = gen(distinct * blk, 11).reshape(distinct, blk)
    src = np.tile(base, (n // distinct + 1, 1))[:n].copy()
    src[:, :8] = np.arange(n, dtype=np.uint64).view(np.uint8).reshape(n, 8) % 10 + 48
    return src.reshape(-1)


class Bench:
    def __init__(self, lib, ctx, reps, warmup, sink):
        self.lib, self.ctx, self.reps, self.warmup, self.sink = lib, ctx, reps, warmup, sink
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        ok(hip.hipEventCreate(C.byref(self.e0)))
        ok(hip.hipEventCreate(C.byref(self.e1)))

    def time(self, legs, calls=1):
        """legs: name -> callable that enqueues one call on the null stream.  Returns name -> (device ms per call, host wall ms per call) lists"""
        dev = {k: [] for k in legs}
        wall = {k: [] for k in legs}
        for r in range(self.warmup + self.reps):
            for k, f in legs.items():
                ok(hip.hipDeviceSynchronize())
                t0 = time.perf_counter()
                ok(hip.hipEventRecord(self.e0, None))
                for _ in range(calls):
                    f()
                ok(hip.hipEventRecord(self.e1, None))
                ok(hip.hipEventSynchronize(self.e1))
                t1 = time.perf_counter()
                ms = C.c_float()
                ok(hip.hipEventElapsedTime(C.byref(ms), self.e0, self.e1))
                if r >= self.warmup:
                    dev[k].append(ms.value / calls)
                    wall[k].append((t1 - t0) * 1e3 / calls)
        return dev, wall

    def report(self, row, what, direction, dev, wall, same, base):
        b = statistics.median(dev[base])
        for k in dev:
            m = statistics.median(dev[k])
            line = json.dumps({"row": row, "what": what, "direction": direction, "leg": k, "ms": round(m, 4), "ms_min": round(min(dev[k]), 4),
                               "ms_max": round(max(dev[k]), 4), "scatter_pct": round(100.0 * (max(dev[k]) - min(dev[k])) / m, 1),
                               "host_ms": round(statistics.median(wall[k]), 4), base + "_over_this": round(b / m, 3), "same_output": same[k]})
            print(line, flush=True)
            if self.sink:
                self.sink.write(line + "\n")
                self.sink.flush()


def run_shape(B, row, what, src, n, blk, dicts, ids, against, calls=1):
    """both directions of one batch: the set entries and `against` ("shared": K = 1, the *_shared_dict entries; "ex": per-block arrays)"""
    lib, ctx = B.lib, B.ctx
    cap1 = 20 + blk * 110 // 100
    d_src = Dev(src)
    in_off, in_len = Dev(np.arange(n, dtype=np.uint64) * blk), Dev(np.full(n, blk, np.uint32))
    c_off, c_cap = Dev(np.arange(n, dtype=np.uint64) * cap1), Dev(np.full(n, cap1, np.uint32))
    d_ids = Dev(np.asarray(ids, np.uint32))
    flat = np.concatenate(dicts)
    lens = np.array([len(d) for d in dicts], np.uint32)
    offs = (np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint64)
    d_dict = Dev(flat)
    st_h = C.c_void_p()
    ok(lib.lz4flex_dict_set_create(ctx, C.c_void_p(flat.ctypes.data), C.c_void_p(offs.ctypes.data), C.c_void_p(lens.ctypes.data), len(dicts),
                                   L.MEM_HOST, C.byref(st_h)), "create")
    d_doff, d_dlen = Dev(offs[np.asarray(ids)]), Dev(lens[np.asarray(ids)])
    cx = L.CompressExt(d_dict.p.value, d_doff.p.value, d_dlen.p.value)
    dx = L.DecompressExt(d_dict.p.value, d_doff.p.value, d_dlen.p.value, None, None, 0)
    names = ("set", against)
    comp = {k: (Dev(size=n * cap1), Dev(size=4 * n), Dev(size=4 * n)) for k in names}

    def enc(k):
        out, ol, st = comp[k]
        if k == "set":
            rc = lib.lz4flex_compress_batch_dict_set(ctx, d_src.p, in_off.p, in_len.p, n, d_ids.p, out.p, c_off.p, c_cap.p, ol.p, st.p, st_h, L.MEM_DEVICE, None)
        elif k == "shared":
            rc = lib.lz4flex_compress_batch_shared_dict(ctx, d_src.p, in_off.p, in_len.p, n, out.p, c_off.p, c_cap.p, ol.p, st.p, d_dict.p, int(lens[0]),
                                                        L.MEM_DEVICE, None)
        else:
            rc = lib.lz4flex_compress_batch_ex(ctx, d_src.p, in_off.p, in_len.p, None, n, out.p, c_off.p, c_cap.p, ol.p, st.p, C.byref(cx), L.MEM_DEVICE, None)
        ok(rc, k)

    dev, wall = B.time({k: (lambda k=k: enc(k)) for k in names}, calls)
    ref_len, ref = comp[against][1].get(np.uint32), comp[against][0].get()
    same = {}
    for k in names:
        ol, st = comp[k][1].get(np.uint32), comp[k][2].get(np.int32)
        got = comp[k][0].get() if k != against else ref
        idx = (np.arange(n, dtype=np.int64) * cap1)[:, None] + np.arange(cap1)[None, :] if n * cap1 < (1 << 27) else None
        eq = bool((st == 0).all()) and bool((ol == ref_len).all())
        if eq and idx is not None:
            mask = np.arange(cap1)[None, :] < ol[:, None]
            eq = bool((got[idx][mask] == ref[idx][mask]).all())
        elif eq:
            eq = all(bytes(got[i * cap1:i * cap1 + ol[i]]) == bytes(ref[i * cap1:i * cap1 + ol[i]]) for i in range(0, n, 97))
        same[k] = eq
    B.report(row, what, "compress", dev, wall, same, against)

    back = {k: (Dev(size=n * blk), Dev(size=4 * n), Dev(size=4 * n)) for k in names}
    cb, cl = comp["set"][0], comp["set"][1]

    def dec(k):
        out, ol, st = back[k]
        if k == "set":
            rc = lib.lz4flex_decompress_batch_dict_set(ctx, cb.p, c_off.p, cl.p, n, d_ids.p, out.p, in_off.p, in_len.p, ol.p, st.p, None, st_h, L.MEM_DEVICE, None)
        elif k == "shared":
            rc = lib.lz4flex_decompress_batch_shared_dict(ctx, cb.p, c_off.p, cl.p, n, out.p, in_off.p, in_len.p, ol.p, st.p, None, d_dict.p, int(lens[0]),
                                                          L.MEM_DEVICE, None)
        else:
            rc = lib.lz4flex_decompress_batch_ex(ctx, cb.p, c_off.p, cl.p, n, out.p, in_off.p, in_len.p, ol.p, st.p, None, C.byref(dx), L.MEM_DEVICE, None)
        ok(rc, k)

    dev, wall = B.time({k: (lambda k=k: dec(k)) for k in names}, calls)
    same = {k: bool((back[k][2].get(np.int32) == 0).all()) and bool((back[k][0].get() == src).all()) for k in names}
    B.report(row, what, "decompress", dev, wall, same, against)
    ok(hip.hipDeviceSynchronize())
    lib.lz4flex_dict_set_free(st_h)
    for group in (comp, back):
        for t in group.values():
            for d in t:
                d.free()
    for d in (d_src, in_off, in_len, c_off, c_cap, d_ids, d_dict, d_doff, d_dlen):
        d.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lib = L.load()
    ctx = C.c_void_p()
    ok(lib.lz4flex_ctx_create(C.byref(ctx), -1), "ctx")
    ok(lib.lz4flex_set_tuning(ctx, b"compress_mode", 0))
    sink = open(args.out, "a") if args.out else None
    B = Bench(lib, ctx, args.reps, args.warmup, sink)
    log_dicts = [log_bytes(32768, 100 + i).copy() for i in range(4)]
    json_dict = json_bytes(32768, 200).copy()
    if args.only in (0, 1):
        n = 65536
        run_shape(B, 1, "K=1, 65536 x 4 KiB log records", tiled(log_bytes, n, 4096, 2048), n, 4096, log_dicts[:1], np.zeros(n, np.int64), "shared")
        n = 16384
        run_shape(B, 1, "K=1, 16384 x 64 KiB JSON tiles", tiled(json_bytes, n, 65536, 64), n, 65536, [json_dict], np.zeros(n, np.int64), "shared")
    if args.only in (0, 2):
        for n in (256, 1024):
            run_shape(B, 2, "K=1, %d x 4 KiB log records, 20 calls in a row" % n, tiled(log_bytes, n, 4096, n), n, 4096, log_dicts[:1],
                      np.zeros(n, np.int64), "shared", calls=20)
    if args.only in (0, 3):
        n = 65536
        run_shape(B, 3, "K=4, 65536 x 4 KiB log records, ids interleaved", tiled(log_bytes, n, 4096, 2048), n, 4096, log_dicts, np.arange(n) % 4, "ex")
    lib.lz4flex_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
