"""tools/paged_append_bench.py -- appends to paged streams (lz4_paged_append.hip: lz4flex_paged_append) on device-resident tables, next to
what the append is made of and to what a caller did before it existed.  The legs of a workload ALTERNATE inside one session; every leg is
one call between two device synchronisations, timed on the host clock; median, minimum and maximum of --reps rounds after --warmup rounds.
No time is a pass condition.

Workloads: 16 384 x 64 KiB JSON tiles in 4 KiB pages; 65 536 x 4 KiB log records in 1 KiB pages (compress_mode 0, default windows).  Each
is paged once into a table with room for the grown streams, then every stream is appended by 256 bytes, by one page's worth and by 16 KiB.
Legs, per add length A:
  append     lz4flex_paged_append: the tail page of every stream reopened, the new bytes behind it.  The tables and the tail pages are
             put back before every timed call, outside the timing, so that every call does the same work
  tail_add   lz4flex_compress_paged over the same `tail ++ add` streams, cut from the source: what the append costs without the reopen
             (the tail decode, the copy and the fixed launches in front of the rounds)
  repage     lz4flex_compress_paged over the whole grown streams from byte 0: what a caller does today
max_rounds is lz4flex_paged_rounds_bound of the longest stream the leg encodes (tail ++ add, or the grown stream): every leg enqueues
exactly that many rounds.  The append's result is decoded and compared with the source first.

usage: python tools/paged_append_bench.py [--reps 5] [--warmup 2] [--shapes 0,1] [--out profiles/r26_paged_append.txt]   (one JSON line per leg)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dict_set_bench import json_bytes, log_bytes, tiled  # noqa: E402
from lz4_flex_amd import _lib as L  # noqa: E402
from lz4_flex_amd import block  # noqa: E402

SHAPES = [("JSON tiles", json_bytes, 16384, 65536, 256, 4096), ("log records", log_bytes, 65536, 4096, 1024, 1024)]
GROW = 16384                                # the longest add


def emit(sink, row):
    line = json.dumps(row)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


def shape(args, sink, what, gen, n, blk, distinct, P):
    import torch
    dev = torch.device("cuda", 0)
    lib = L.load()
    stride = blk + GROW
    d_src = torch.from_numpy(tiled(gen, n, stride, distinct)).to(dev)
    at = torch.arange(n, dtype=torch.int64, device=dev) * stride
    block.set_compress_mode("fast")
    wmin, wmax = 4 * P, max(4 * P, 65536)
    cap = int(lib.lz4flex_paged_pages_bound(stride, P))
    paged = block.compress_paged_device(d_src, at, torch.full((n,), blk, dtype=torch.int64), P, page_cap=torch.full((n,), cap, dtype=torch.int64))
    torch.cuda.synchronize()
    assert (paged.status == 0).all()
    k0 = paged.n_pages.to(torch.int64)
    tail_idx = paged.page_off[:n] + k0 - 1
    base = paged.page_src.to(torch.int64)[tail_idx]
    T = blk - base
    saved = [t.clone() for t in (paged.n_pages, paged.in_done, paged.page_len, paged.page_src)]
    saved_tail = paged.pages.view(-1, P)[tail_idx].clone()
    longest_tail = int(T.max())

    def restore():
        for dst, src in zip((paged.n_pages, paged.in_done, paged.page_len, paged.page_src), saved):
            dst.copy_(src)
        paged.pages.view(-1, P)[tail_idx] = saved_tail

    i32 = lambda m: torch.zeros(m, dtype=torch.int32, device=dev)     # noqa: E731
    p = lambda x: C.c_void_p(x.data_ptr())     # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    legs, facts, keep = {}, {}, []

    def paged_leg(name, in_off, in_len, rounds):
        """one lz4flex_compress_paged into a table of its own, `cap` entries per stream"""
        off = torch.arange(n + 1, dtype=torch.int64, device=dev) * cap
        file = torch.empty(n * cap * P, dtype=torch.uint8, device=dev)
        arr = [i32(n * cap), i32(n * cap), i32(n), i32(n), i32(n)]
        d_len = in_len.to(torch.int32).contiguous()
        offered = int(torch.clamp(in_len, max=wmax).sum())
        scratch_cap = int(lib.lz4flex_compress_packed_scratch_bound(offered, n, 0))
        scratch = torch.empty(scratch_cap + 1, dtype=torch.uint8, device=dev)
        work = torch.empty(int(lib.lz4flex_compress_paged_work_size(n)), dtype=torch.uint8, device=dev)
        keep.append((off, file, arr, d_len, in_off, scratch, work))

        def call():
            rc = lib.lz4flex_compress_paged(None, p(d_src), p(in_off), p(d_len), n, P, 0, 0, rounds, p(file), p(off), *[p(a) for a in arr], p(scratch),
                                            scratch_cap, p(work), L.MEM_DEVICE, stream)
            assert rc == 0, L.last_error()
        legs[name] = call
        facts[name] = {"rounds": rounds, "bytes_encoded_per_stream": round(float(in_len.double().mean()), 1), "_status": arr[4], "_n_pages": arr[2]}

    for A in (256, P, GROW):
        add_off = (at + blk).contiguous()
        add_len = torch.full((n,), A, dtype=torch.int32, device=dev)
        V = T + A
        rounds = int(lib.lz4flex_paged_rounds_bound(longest_tail + A, P, 0, 0))
        stage_cap = int(((V + 63) // 64 * 64).sum())
        scratch_cap = int(lib.lz4flex_compress_packed_scratch_bound(int(torch.clamp(V, max=wmax).sum()), n, 0))
        stage = torch.empty(stage_cap + 64, dtype=torch.uint8, device=dev)
        scratch = torch.empty(scratch_cap + 1, dtype=torch.uint8, device=dev)
        work = torch.empty(int(lib.lz4flex_paged_append_work_size(n)), dtype=torch.uint8, device=dev)
        status, stage_off, tail_src = i32(n), torch.zeros(n, dtype=torch.int64, device=dev), i32(n)
        keep.append((add_off, add_len, stage, scratch, work, status, stage_off, tail_src))

        def call(add_off=add_off, add_len=add_len, rounds=rounds, stage=stage, stage_cap=stage_cap, scratch=scratch, scratch_cap=scratch_cap,
                 work=work, status=status, stage_off=stage_off, tail_src=tail_src):
            rc = lib.lz4flex_paged_append(None, p(d_src), p(add_off), p(add_len), n, P, 0, 0, rounds, p(paged.pages), p(paged.page_off),
                                          p(paged.page_len), p(paged.page_src), p(paged.n_pages), p(paged.in_done), p(status), p(stage), stage_cap,
                                          p(stage_off), p(tail_src), p(scratch), scratch_cap, p(work), L.MEM_DEVICE, stream)
            assert rc == 0, L.last_error()
        legs["append %d" % A] = call
        facts["append %d" % A] = {"rounds": rounds, "bytes_encoded_per_stream": round(float(V.double().mean()), 1), "_status": status,
                                  "_n_pages": paged.n_pages, "_restore": True}
        paged_leg("tail_add %d" % A, (at + base).contiguous(), V, rounds)
        paged_leg("repage %d" % A, at, torch.full((n,), blk + A, dtype=torch.int64, device=dev),
                  int(lib.lz4flex_paged_rounds_bound(blk + A, P, 0, 0)))
        # the append once, checked against the source
        restore()
        call()
        torch.cuda.synchronize()
        assert (status == 0).all(), status[status != 0][:4]
        out, out_off, out_len, st = block.decompress_paged_device(paged)
        torch.cuda.synchronize()
        assert (st == 0).all() and bool((out.view(n, blk + A) == d_src.view(n, stride)[:, :blk + A]).all()), "the appended streams differ from the source"
        facts["append %d" % A]["pages_per_stream_after"] = round(float(paged.n_pages.double().mean()), 3)
    ms = {name: [] for name in legs}
    for rnd in range(args.warmup + args.reps):
        for name, call in legs.items():
            if facts[name].get("_restore"):
                restore()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            if rnd >= args.warmup:
                ms[name].append(1000.0 * (time.perf_counter() - t0))
            assert (facts[name]["_status"] == 0).all(), name
    restore()
    for name, v in ms.items():
        med = statistics.median(v)
        A = name.split()[1]
        row = {"shape": "%d x %d %s in %d-byte pages" % (n, blk, what, P), "leg": name, "ms": round(med, 4), "ms_min": round(min(v), 4),
               "ms_max": round(max(v), 4), "pages_per_stream_before": round(float(k0.double().mean()), 3),
               "tail_bytes_per_stream": round(float(T.double().mean()), 1)}
        row.update({a: b for a, b in facts[name].items() if not a.startswith("_")})
        if name.startswith("append"):
            row["append_over_tail_add"] = round(med / statistics.median(ms["tail_add " + A]), 3)
            row["repage_over_append"] = round(statistics.median(ms["repage " + A]) / med, 3)
        emit(sink, row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sink = open(args.out, "a") if args.out else None
    for s in (int(v) for v in args.shapes.split(",")):
        shape(args, sink, *SHAPES[s])


if __name__ == "__main__":
    main()
