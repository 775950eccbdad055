"""tools/paged_read_bench.py -- byte-range reads of paged streams (lz4_paged_read.hip: lz4flex_paged_read_ranges) on device-resident
tables, next to the read side the library had before it: block.decompress_paged_device, a torch composition over the page table with one
lz4flex_decompress_batch and a host synchronisation.  The legs of a workload ALTERNATE inside one session; every leg is one call between
two device synchronisations, timed on the host clock (the yardstick synchronises inside, so device events would flatter it); median,
minimum and maximum of --reps rounds after --warmup rounds.  No time is a pass condition.

Workloads: 16 384 x 64 KiB JSON tiles in 4 KiB pages; 65 536 x 4 KiB log records in 1 KiB pages (compress_mode 0, default windows,
capacities of lz4flex_paged_pages_bound).  Legs:
  whole            every stream as ONE range (off 0, len 0xFFFFFFFF), max_items = the touched pages
  torch_whole      block.decompress_paged_device on the same tables: the yardstick, its synchronisation included
  4K x 1024, 4K x 65536   random ranges of 4 096 bytes (clipped at the stream's end), max_items = the touched pages
  64B x 65536      random ranges of 64 bytes
  4K x ... items x4       the 4 KiB legs with max_items at four times the need: what empty decoder slots cost
Every row carries the touched pages, the share of ranges with a head and the head scratch in use; the buffers are allocated once, outside
the timed calls.  The whole-stream leg's bytes are compared with the source first.

usage: python tools/paged_read_bench.py [--reps 5] [--warmup 2] [--shapes 0,1] [--out profiles/r25_paged_read.txt]   (one JSON line per leg)"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dict_set_bench import json_bytes, log_bytes, tiled  # noqa: E402
from lz4_flex_amd import _lib as L  # noqa: E402
from lz4_flex_amd import block  # noqa: E402

SHAPES = [("JSON tiles", json_bytes, 16384, 65536, 256, 4096), ("log records", log_bytes, 65536, 4096, 1024, 1024)]
WHOLE = 0xFFFFFFFF


def emit(sink, row):
    line = json.dumps(row)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


def located(tab, sid, off, length):
    """(touched pages, ranges with a head, head scratch bytes) of ranges over the host copy of the tables (every stream owns `cap` entries)"""
    src2d, k, done = tab
    S = done[sid]
    n = np.where(off < S, np.minimum(length, S - off), 0)
    live = n > 0
    rows = src2d[sid]
    last = off + np.maximum(n, 1) - 1
    j0 = (rows <= off[:, None]).sum(1) - 1
    j1 = (rows <= last[:, None]).sum(1) - 1
    a = rows[np.arange(sid.size), np.maximum(j0, 0)]
    b = np.where(j0 + 1 < k[sid], rows[np.arange(sid.size), np.minimum(j0 + 1, rows.shape[1] - 1)], S)
    head = live & (a < off)
    head_bytes = np.where(head, np.minimum(b, off + n) - a, 0)
    return int(np.where(live, j1 - j0 + 1, 0).sum()), int(head.sum()), int(((head_bytes + 63) // 64 * 64).sum())


def shape(args, sink, what, gen, n, blk, distinct, P):
    import torch
    dev = torch.device("cuda", 0)
    lib = L.load()
    src = tiled(gen, n, blk, distinct)
    d_src = torch.from_numpy(src.reshape(-1)).to(dev)
    in_off = torch.arange(n, dtype=torch.int64) * blk
    in_len = torch.full((n,), blk, dtype=torch.int64)
    block.set_compress_mode("fast")
    paged = block.compress_paged_device(d_src, in_off, in_len, P)
    torch.cuda.synchronize()
    assert (paged.status == 0).all()
    cap = int(lib.lz4flex_paged_pages_bound(blk, P))
    k = paged.n_pages.cpu().numpy().astype(np.int64)
    done = paged.in_done.cpu().numpy().astype(np.int64)
    src2d = paged.page_src.cpu().numpy().astype(np.int64).reshape(n, cap)
    src2d = np.where(np.arange(cap)[None, :] < k[:, None], src2d, 1 << 40)
    tab = (src2d, k, done)
    entries = n * cap
    rng = np.random.default_rng(5)

    def ranges(m, length):
        sid = rng.integers(0, n, m)
        off = (rng.random(m) * np.maximum(done[sid] - min(length, blk) + 1, 1)).astype(np.int64)
        return sid, off, np.full(m, length, np.int64)

    legs, facts = {}, {}

    def add(name, sid, off, length, items_factor=1):
        m = sid.size
        touched, heads, head_scratch = located(tab, sid, off, length)
        max_items = touched * items_factor
        room = np.where(off < done[sid], np.minimum(length, done[sid] - off), 0)
        out_off = torch.from_numpy(np.cumsum(room) - room).to(dev)
        out = torch.empty(max(int(room.sum()), 1), dtype=torch.uint8, device=dev)
        t = [torch.from_numpy(a.astype(np.uint32).view(np.int32)).to(dev) for a in (sid, off, length)]
        out_len, status = torch.zeros(m, dtype=torch.int32, device=dev), torch.zeros(m, dtype=torch.int32, device=dev)
        scratch = torch.empty(head_scratch + 64, dtype=torch.uint8, device=dev)
        work = torch.empty(int(lib.lz4flex_paged_read_work_size(m, max_items)), dtype=torch.uint8, device=dev)
        keep = (t, out, out_off, out_len, status, scratch, work)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        p = lambda x: C.c_void_p(x.data_ptr())     # noqa: E731

        def call():
            rc = lib.lz4flex_paged_read_ranges(None, p(paged.pages), P, p(paged.page_off), p(paged.page_len), p(paged.page_src), p(paged.n_pages),
                                               p(paged.in_done), n, p(t[0]), p(t[1]), p(t[2]), m, p(out), p(out_off), p(out_len), p(status),
                                               max_items, p(scratch), head_scratch, p(work), L.MEM_DEVICE, stream)
            assert rc == 0, L.last_error()
        legs[name] = call
        facts[name] = {"ranges": m, "touched_pages": touched, "max_items": max_items, "head_share": round(heads / m, 4), "head_scratch": head_scratch,
                       "bytes": int(room.sum()), "_keep": keep}
        return keep

    whole = add("whole", np.arange(n), np.zeros(n, np.int64), np.full(n, WHOLE, np.int64))
    legs["whole"]()
    torch.cuda.synchronize()
    assert (whole[4] == 0).all() and bool((whole[1][:n * blk] == d_src[:n * blk]).all()), "whole-stream read differs from the source"
    legs["torch_whole"] = lambda: block.decompress_paged_device(paged)
    facts["torch_whole"] = {"ranges": n, "touched_pages": int(k.sum()), "bytes": int(done.sum())}
    for m in (1024, 65536):
        r = ranges(m, 4096)
        add("4K x %d" % m, *r)
        add("4K x %d items x4" % m, *r, items_factor=4)
    add("64B x 65536", *ranges(65536, 64))
    for name, call in legs.items():                    # every leg once, checked
        call()
        torch.cuda.synchronize()
        if "_keep" in facts[name]:
            st = facts[name]["_keep"][4]
            assert (st == 0).all(), (name, st[st != 0][:4])
    ms = {name: [] for name in legs}
    for rnd in range(args.warmup + args.reps):
        for name, call in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            if rnd >= args.warmup:
                ms[name].append(1000.0 * (time.perf_counter() - t0))
    for name, v in ms.items():
        med = statistics.median(v)
        row = {"shape": "%d x %d %s in %d-byte pages" % (n, blk, what, P), "leg": name, "ms": round(med, 4), "ms_min": round(min(v), 4),
               "ms_max": round(max(v), 4), "pages_per_stream": round(float(k.mean()), 3), "entries": entries}
        row.update({a: b for a, b in facts[name].items() if a != "_keep"})
        row["us_per_touched_page"] = round(1000.0 * med / max(row["touched_pages"], 1), 4)
        if name == "whole":
            row["torch_whole_over_whole"] = round(statistics.median(ms["torch_whole"]) / med, 3)
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
