"""tools/shared_dict_decode_bench.py -- lz4flex_decompress_batch_shared_dict next to the other ways to decode the same records, on
device-resident batches with one 32 KiB dictionary.  The legs ALTERNATE inside one session; each round times one call of every leg with
device events, after --warmup rounds; the median, minimum and maximum of --reps rounds are reported per leg, and every leg's output is
compared with the input.

  shapes    (a) 16 384 x 64 KiB JSON tiles     (b) 65 536 x 4 KiB log records      (the workloads of tools/dict_bench.py)
  encoders  fast: lz4flex_compress_batch_shared_dict, compress_mode fast (its matches reach 32 KiB into the dictionary)
            oracle: the reference's compress_with_dict on the CPU (oracle/; its matches reach 64 KiB)
  legs      shared      lz4flex_decompress_batch_shared_dict (the sequence decoder's dictionary form)
            per_block   lz4flex_decompress_batch_ex with dict_off / dict_len arrays that name the dictionary for every block: the baseline
            shared_off  the entry with "decompress_shared_dict" 0 (the reference's order, sixteen lanes per block)
            no_dict     the same records compressed WITHOUT a dictionary (compress_mode fast) through lz4flex_decompress_batch: the floor

usage: python tools/shared_dict_decode_bench.py [--reps 7] [--warmup 2] [--workload a|b|both] [--encoder fast|oracle|both]   (one JSON line per leg)"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dict_bench import p, workload  # noqa: E402
from lz4_flex_amd import _lib as L  # noqa: E402

LEGS = ("per_block", "shared", "shared_off", "no_dict")


def oracle_blocks(src, dic, n, blk, dev):
    """every record compressed by the reference's compress_with_dict (CPU, a few threads: ctypes releases the GIL), packed back to back"""
    import oracle_api as O
    so = os.path.join(ROOT, "oracle", "liblz4flex_oracle.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")], stdout=subprocess.DEVNULL)
    o = O.lib()
    h = src.cpu().numpy()
    d = dic.cpu().numpy().tobytes()
    cap = O.max_out(blk)
    chunk = 256

    def work(c0):
        out = C.create_string_buffer(cap)
        res = []
        for i in range(c0, min(c0 + chunk, n)):
            m = o.lz4o_compress_into_with_dict(h[i * blk:(i + 1) * blk].tobytes(), blk, out, cap, d, len(d))
            assert m >= 0
            res.append(out.raw[:m])
        return res

    with ThreadPoolExecutor(8) as ex:
        blocks = [b for part in ex.map(work, range(0, n, chunk)) for b in part]
    lens = np.array([len(b) for b in blocks], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens[:-1])])
    comp = torch.from_numpy(np.frombuffer(b"".join(blocks) + bytes(64), dtype=np.uint8).copy()).to(dev)
    return comp, torch.from_numpy(offs).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", choices=["a", "b", "both"], default="both")
    ap.add_argument("--encoder", choices=["fast", "oracle", "both"], default="both")
    args = ap.parse_args()
    lib = L.load()
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), -1) == 0
    assert lib.lz4flex_set_tuning(ctx, b"compress_mode", 0) == 0
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    for w in (["a", "b"] if args.workload == "both" else [args.workload]):
        what, src, dic, n, blk = workload(w, dev)
        in_off = torch.arange(n, dtype=torch.int64, device=dev) * blk
        in_len = torch.full((n,), blk, dtype=torch.int32, device=dev)
        cap1 = 20 + blk * 110 // 100
        c_off = torch.arange(n, dtype=torch.int64, device=dev) * cap1
        c_cap = torch.full((n,), cap1, dtype=torch.int32, device=dev)
        d_off = torch.zeros(n, dtype=torch.int64, device=dev)
        d_len = torch.full((n,), dic.numel(), dtype=torch.int32, device=dev)
        dx = L.DecompressExt(dic.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), None, None, 0)

        def compress(with_dict):
            out = torch.zeros(n * cap1, dtype=torch.uint8, device=dev)
            out_len = torch.zeros(n, dtype=torch.int32, device=dev)
            st = torch.zeros(n, dtype=torch.int32, device=dev)
            if with_dict:
                rc = lib.lz4flex_compress_batch_shared_dict(ctx, p(src), p(in_off), p(in_len), n, p(out), p(c_off), p(c_cap), p(out_len), p(st),
                                                            p(dic), dic.numel(), L.MEM_DEVICE, sp)
            else:
                rc = lib.lz4flex_compress_batch(ctx, p(src), p(in_off), p(in_len), None, n, p(out), p(c_off), p(c_cap), p(out_len), p(st),
                                                L.MEM_DEVICE, sp)
            assert rc == 0, (rc, L.last_error())
            torch.cuda.synchronize()
            assert int((st != 0).sum()) == 0, "compress status"
            return out, c_off, out_len

        plain_comp = compress(False)
        for enc in (["fast", "oracle"] if args.encoder == "both" else [args.encoder]):
            comp = compress(True) if enc == "fast" else oracle_blocks(src, dic, n, blk, dev)
            back = {leg: (torch.zeros(n * blk, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                          torch.full((n,), -1, dtype=torch.int32, device=dev)) for leg in LEGS}

            def once(leg):
                out, out_len, st = back[leg]
                cb, co, cl = plain_comp if leg == "no_dict" else comp
                if leg == "per_block":
                    rc = lib.lz4flex_decompress_batch_ex(ctx, p(cb), p(co), p(cl), n, p(out), p(in_off), p(in_len), p(out_len), p(st), None,
                                                         C.byref(dx), L.MEM_DEVICE, sp)
                elif leg == "no_dict":
                    rc = lib.lz4flex_decompress_batch(ctx, p(cb), p(co), p(cl), n, p(out), p(in_off), p(in_len), p(out_len), p(st), None,
                                                      L.MEM_DEVICE, sp)
                else:
                    assert lib.lz4flex_set_tuning(ctx, b"decompress_shared_dict", 1 if leg == "shared" else 0) == 0
                    rc = lib.lz4flex_decompress_batch_shared_dict(ctx, p(cb), p(co), p(cl), n, p(out), p(in_off), p(in_len), p(out_len), p(st),
                                                                  None, p(dic), dic.numel(), L.MEM_DEVICE, sp)
                assert rc == 0, (rc, L.last_error())

            times = {leg: [] for leg in LEGS}
            for r in range(args.warmup + args.reps):
                for leg in LEGS:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    once(leg)
                    e1.record(stream)
                    e1.synchronize()
                    if r >= args.warmup:
                        times[leg].append(e0.elapsed_time(e1))
            assert lib.lz4flex_set_tuning(ctx, b"decompress_shared_dict", 1) == 0
            torch.cuda.synchronize()
            ok = {leg: int((back[leg][2] != 0).sum()) == 0 and bool((back[leg][1] == blk).all()) and bool(torch.equal(back[leg][0], src))
                  for leg in LEGS}
            base = statistics.median(times["per_block"])
            for leg in LEGS:
                ms = statistics.median(times[leg])
                cl = (plain_comp if leg == "no_dict" else comp)[2]
                print(json.dumps({"workload": w, "what": what, "encoder": enc if leg != "no_dict" else "fast, no dictionary", "leg": leg,
                                  "ms": round(ms, 3), "ms_min": round(min(times[leg]), 3), "ms_max": round(max(times[leg]), 3),
                                  "spread_pct": round(100.0 * (max(times[leg]) - min(times[leg])) / ms, 1),
                                  "per_block_over_this": round(base / ms, 3), "GiB_per_s": round(n * blk / 2**30 / (ms / 1e3), 2),
                                  "ratio": round(int(cl.to(torch.int64).sum()) / (n * blk), 4), "output_is_input": ok[leg]}), flush=True)
            del back, comp
            torch.cuda.empty_cache()
        del src, plain_comp
        torch.cuda.empty_cache()
    lib.lz4flex_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
