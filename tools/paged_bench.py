"""tools/paged_bench.py -- the paged streams (lz4_paged.hip: lz4flex_compress_paged) on device-resident data.  Torch-free: device memory,
events and copies through the HIP runtime (ctypes).  The legs of a measurement ALTERNATE inside one session; each round times one call
of every leg with device events after --warmup rounds; median, minimum and maximum of --reps rounds per leg.  No time is a pass condition.

Per workload (16 384 x 64 KiB JSON tiles into 4 KiB pages; 65 536 x 4 KiB log records into 1 KiB pages; compress_mode 0, the default
windows, capacities of lz4flex_paged_pages_bound) the legs are
  paged        ONE lz4flex_compress_paged, MEM_DEVICE, max_rounds = the rounds this data needs (found by a first call at the bound)
  paged_bound  the same call with max_rounds = lz4flex_paged_rounds_bound: the rounds behind the last live stream cost their launches
  host_loop    the same job the way a caller had to write it before: per round the window arrays uploaded, ONE lz4flex_compress_batch_fit,
               out_len / in_used / status read back (a synchronisation), the rule applied on the host (numpy)
  plain        ONE lz4flex_compress_batch of the same streams as whole blocks: the floor
and the row of `paged` carries pages per stream, the fill (sum of page_len / (pages x P)), the offered window bytes / input bytes (the
rule replayed on the results) and paged / (offered ratio x plain): the expectation it is held against is about 1.  The host loop's tables
are compared with the device loop's first (same_as_paged).

usage: python tools/paged_bench.py [--reps 5] [--warmup 2] [--shapes 0,1] [--out profiles/r24_paged.txt]     (one JSON line per leg)"""
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

from dict_set_bench import D2H, H2D, Bench, Dev, hip, json_bytes, log_bytes, ok, tiled  # noqa: E402  (loads libamdhip64 as well)
from lz4_flex_amd import _lib as L  # noqa: E402

SHAPES = [("JSON tiles", json_bytes, 16384, 65536, 256, 4096), ("log records", log_bytes, 65536, 4096, 1024, 1024)]


def emit(sink, row):
    line = json.dumps(row)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


def stats(ms):
    m = statistics.median(ms)
    return {"ms": round(m, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "scatter_pct": round(100.0 * (max(ms) - min(ms)) / m, 1)}


def put(dev, a):
    ok(hip.hipMemcpy(dev.p, C.c_void_p(a.ctypes.data), a.nbytes, H2D))


def page_bytes(dev, e, P, length):
    out = np.empty(max(length, 1), np.uint8)
    ok(hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(dev.p.value + e * P), length, D2H))
    return out[:length].tobytes()


def replay(in_len, first, n_pages, page_src, in_done, wmin, wmax):
    """(offered window bytes, rounds per stream) of finished streams, the rule replayed on their tables: a commit at pos that used `used`
    bytes was offered min(W, left) bytes after a retry at every W that `used` reaches with more of the stream behind the window"""
    n = in_len.size
    W = np.full(n, wmin, np.int64)
    offered, rounds = np.zeros(n, np.int64), n_pages.astype(np.int64).copy()
    for j in range(int(n_pages.max()) if n else 0):
        on = n_pages > j
        e = np.where(on, first + j, 0)
        pos = page_src[e].astype(np.int64)
        end = np.where(n_pages > j + 1, page_src[np.where(n_pages > j + 1, e + 1, 0)], in_done).astype(np.int64)
        left, used = in_len - pos, end - pos
        while True:
            w = np.minimum(W, left)
            offered += np.where(on, w, 0)
            again = on & (used >= w) & (w < left) & (W < wmax)
            if not again.any():
                break
            W = np.where(again, np.minimum(2 * W, wmax), W)
            rounds += again
            on = again
    return offered, rounds


def shape(B, sink, what, gen, n, blk, distinct, P):
    lib, ctx = B.lib, B.ctx
    src = tiled(gen, n, blk, distinct)
    d_src = Dev(src)
    in_len = np.full(n, blk, np.uint32)
    in_off = np.arange(n, dtype=np.uint64) * blk
    wmin, wmax = 4 * P, max(4 * P, 65536)
    cap = int(lib.lz4flex_paged_pages_bound(blk, P))
    page_off = np.arange(n + 1, dtype=np.uint64) * cap
    entries = n * cap
    bound = int(lib.lz4flex_paged_rounds_bound(blk, P, 0, 0))
    d_off, d_len, d_poff = Dev(in_off), Dev(in_len), Dev(page_off)
    file, p_len, p_src = Dev(size=entries * P), Dev(size=4 * entries), Dev(size=4 * entries)
    n_pages, in_done, status = Dev(size=4 * n), Dev(size=4 * n), Dev(size=4 * n)
    scratch_cap = int(lib.lz4flex_compress_packed_scratch_bound(n * min(blk, wmax), n, 0))
    scratch, work = Dev(size=scratch_cap), Dev(size=int(lib.lz4flex_compress_paged_work_size(n)))
    ok(lib.lz4flex_set_tuning(ctx, b"compress_mode", 0))

    def paged(rounds):
        ok(lib.lz4flex_compress_paged(ctx, d_src.p, d_off.p, d_len.p, n, P, 0, 0, rounds, file.p, d_poff.p, p_len.p, p_src.p, n_pages.p, in_done.p,
                                      status.p, scratch.p, scratch_cap, work.p, L.MEM_DEVICE, None), "paged")

    paged(bound)
    ok(hip.hipDeviceSynchronize())
    k, done, st = n_pages.get(np.uint32).astype(np.int64), in_done.get(np.uint32), status.get(np.int32)
    t_len, t_src = p_len.get(np.uint32), p_src.get(np.uint32)
    assert (st == 0).all() and (done == in_len).all() and (k <= cap).all()
    first = page_off[:n].astype(np.int64)
    offered, per_stream = replay(in_len.astype(np.int64), first, k, t_src, done, wmin, wmax)
    need = int(per_stream.max())
    committed = (np.arange(entries) - np.repeat(first, cap)) < np.repeat(k, cap)
    facts = {"page_size": P, "window_min": wmin, "window_max": wmax, "rounds_needed": need, "rounds_bound": bound,
             "pages_per_stream": round(float(k.mean()), 3), "pages_bound_per_stream": cap,
             "fill": round(float(t_len[committed].sum()) / (float(k.sum()) * P), 4),
             "offered_over_input": round(float(offered.sum()) / float(in_len.sum()), 4)}

    # the host loop: the arrays of a round uploaded, one fit batch, its results read back, the rule in numpy
    w_off, w_len, o_off, o_cap = Dev(size=8 * n), Dev(size=4 * n), Dev(size=8 * n), Dev(size=4 * n)
    r_len, r_used, r_st = Dev(size=4 * n), Dev(size=4 * n), Dev(size=4 * n)
    file2 = Dev(size=entries * P)
    fit_work = Dev(size=int(lib.lz4flex_compress_fit_work_size(n)))
    host = {}

    def host_loop():
        pos, W, kk = np.zeros(n, np.int64), np.full(n, wmin, np.int64), np.zeros(n, np.int64)
        live = in_len > 0
        h_len, h_src = np.zeros(entries, np.uint32), np.zeros(entries, np.uint32)
        rounds = sent = 0
        while live.any():
            rounds += 1
            w = np.where(live, np.minimum(W, in_len - pos), 0)
            sent += int(w.sum())
            put(w_off, (in_off + np.where(live, pos, 0).astype(np.uint64)).astype(np.uint64))
            put(w_len, w.astype(np.uint32))
            put(o_off, np.where(live, (first + kk) * P, 0).astype(np.uint64))
            put(o_cap, np.where(live, P, 0).astype(np.uint32))
            ok(lib.lz4flex_compress_batch_fit(ctx, d_src.p, w_off.p, w_len.p, n, scratch.p, scratch_cap, file2.p, o_off.p, o_cap.p, r_len.p, r_used.p,
                                              r_st.p, fit_work.p, L.MEM_DEVICE, None), "compress_fit")
            ln, used, rs = r_len.get(np.uint32), r_used.get(np.uint32).astype(np.int64), r_st.get(np.int32)      # (the synchronisation)
            assert (rs[live] == 0).all()
            retry = live & (used == w) & (pos + w < in_len) & (W < wmax)
            commit = live & ~retry
            W = np.where(retry, np.minimum(2 * W, wmax), W)
            e = (first + kk)[commit]
            h_len[e], h_src[e] = ln[commit], pos[commit].astype(np.uint32)
            pos = pos + np.where(commit, used, 0)
            kk = kk + commit
            live = live & (pos < in_len)
        host.update(rounds=rounds, offered=sent, n_pages=kk, page_len=h_len, page_src=h_src)

    host_loop()
    same = bool((host["n_pages"] == k).all() and (host["page_len"][committed] == t_len[committed]).all()
                and (host["page_src"][committed] == t_src[committed]).all())
    for e in np.nonzero(committed)[0][::max(int(committed.sum()) // 257, 1)]:              # a sample of the pages, byte for byte
        same = same and page_bytes(file, int(e), P, int(t_len[e])) == page_bytes(file2, int(e), P, int(t_len[e]))
    assert host["rounds"] == need and host["offered"] == int(offered.sum()), (host["rounds"], need, host["offered"], int(offered.sum()))

    cap1 = 20 + blk * 110 // 100
    c_off, c_cap = Dev(np.arange(n, dtype=np.uint64) * cap1), Dev(np.full(n, cap1, np.uint32))
    comp, c_len, c_st = Dev(size=n * cap1), Dev(size=4 * n), Dev(size=4 * n)

    def plain():
        ok(lib.lz4flex_compress_batch(ctx, d_src.p, d_off.p, d_len.p, None, n, comp.p, c_off.p, c_cap.p, c_len.p, c_st.p, L.MEM_DEVICE, None), "compress")

    plain()
    ok(hip.hipDeviceSynchronize())
    assert (c_st.get(np.int32) == 0).all()
    facts["plain_ratio"] = round(float(c_len.get(np.uint32).sum()) / float(in_len.sum()), 4)
    facts["paged_ratio"] = round(float(k.sum()) * P / float(in_len.sum()), 4)
    dev, wall = B.time({"paged": lambda: paged(need), "paged_bound": lambda: paged(bound), "host_loop": host_loop, "plain": plain})
    med = {name: statistics.median(v) for name, v in dev.items()}
    for name, ms in dev.items():
        row = {"shape": "%d x %d %s -> %d-byte pages" % (n, blk, what, P), "leg": name}
        row.update(stats(ms), wall_ms=round(statistics.median(wall[name]), 4))
        if name == "paged":
            row.update(facts, over_offered_times_plain=round(med["paged"] / (facts["offered_over_input"] * med["plain"]), 3),
                       host_loop_over_paged=round(med["host_loop"] / med["paged"], 3),
                       host_loop_minus_paged_ms_per_round=round((med["host_loop"] - med["paged"]) / need, 4))
        if name == "host_loop":
            row.update(same_as_paged=same, rounds=host["rounds"])
        emit(sink, row)
    for d in (d_src, d_off, d_len, d_poff, file, p_len, p_src, n_pages, in_done, status, scratch, work, w_off, w_len, o_off, o_cap, r_len, r_used, r_st,
              file2, fit_work, c_off, c_cap, comp, c_len, c_st):
        d.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sink = open(args.out, "a") if args.out else None
    lib = L.load()
    ctx = C.c_void_p()
    ok(lib.lz4flex_ctx_create(C.byref(ctx), -1), "ctx")
    B = Bench(lib, ctx, args.reps, args.warmup, sink)
    for s in (int(v) for v in args.shapes.split(",")):
        shape(B, sink, *SHAPES[s])
    lib.lz4flex_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
