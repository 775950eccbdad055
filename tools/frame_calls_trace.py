#!/usr/bin/env python3
"""What the frame layer's six entry points put on the device, as a list two builds can be compared by: kernel names in order, memory
copies with direction and bytes.

  frame_calls_trace.py run          calls lz4flex_frame_compress_many, lz4flex_frame_decompress_many, lz4flex_frame_index_create,
                                    lz4flex_frame_read_ranges, lz4flex_frame_compress_sharded and lz4flex_frame_decompress_sharded (one
                                    rank, no communicator), each again where a second shape has other columns, on three streams of
                                    two 64 KiB blocks and a 1 000-byte tail: text, random bytes, text.  Run it under
                                        rocprofv3 --kernel-trace --memory-copy-trace --output-format json -d DIR -o trace -- python ... run
                                    (no counters in that run); LZ4FLEX_LIB picks the build.
  frame_calls_trace.py run-stream   a second scenario, traced the same way: the streaming FrameEncoder and FrameDecoder and the two one-shot
                                    calls, once each, on a Linked frame of eight writes with a flush behind each (65536 x 3, 1000,
                                    65536, 30000, 65536 x 2 bytes) and on an Independent frame of five blocks and a 1 000-byte tail:
                                    encoded in compress_mode fast and exact, each frame read back with read(65536) and read(1 MiB).
  frame_calls_trace.py list DIR    the trace as one line per kernel ("K name") and per copy ("C direction bytes"), by start time.
                                    Small pageable copies are staged by the runtime and appear as its copy kernel, without a size:
  frame_calls_trace.py copies LOG   every hipMemcpy* call of a `run` whose stderr went to LOG under AMD_LOG_LEVEL=3 (the HIP
                                    runtime's own call log), in call order: "M direction bytes".

The set-up (torch's own copies and fills) is part of both lists and the same in both."""
import ctypes as C
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
BS = 65536
SIZE = 2 * BS + 1000


def run():
    import numpy as np
    import torch
    import oracle_api as O
    from lz4_flex_amd import _lib as L, block, frame as F
    lib = L.load()
    text = O.fixture_plain("compression_65k") + O.fixture_plain("compression_66k_JSON")
    rnd = np.random.default_rng(25).integers(0, 256, SIZE, dtype=np.uint8).tobytes()
    streams = [(text + text)[:SIZE], rnd, (text[5000:] + text)[:SIZE]]
    assert all(len(v) == SIZE for v in streams)
    for mode, exact in ((0, False), (1, False), (1, True)):        # Independent; Linked; Linked with the reference-exact encoder's chain columns
        info = F.FrameInfo(block_mode=F.BlockMode(mode), block_size=F.BlockSize.Max64KB, block_checksums=True, content_checksum=True)
        block.set_compress_mode("exact" if exact else "fast")
        try:
            frames = F.compress_frames(streams, info)
        finally:
            block.set_compress_mode("fast")
        assert F.decompress_frames(frames, [SIZE] * 3) == streams
        if mode == 0:
            seek = frames
    both = [seek[0], frames[1]]                                     # an Independent and a Linked frame in one call
    assert F.decompress_frames(both, [SIZE] * 2) == streams[:2]
    for f, s in zip(seek[:2], streams):                             # compressed blocks with checksums; stored blocks
        for src in (f, torch.from_numpy(np.frombuffer(f, np.uint8).copy()).cuda()):
            with F.FrameIndex(src) as ix:
                for ranges in ([(0, 0), (SIZE, 5)], [(BS, 3000)], [(BS + 100, 3000)], [(7, 100000), (BS - 1, 2), (SIZE - 10, 50)]):
                    assert ix.read_ranges(ranges) == [s[o:o + n] for o, n in ranges]
    ctx = C.c_void_p()
    assert lib.lz4flex_ctx_create(C.byref(ctx), 0) == 0
    for s in streams[:2]:                                           # one rank, no communicator: the rank's own blocks, then back
        fic = L.FrameInfoC(0, 0, 4, 0, 1, 0, 0)
        src = torch.from_numpy(np.frombuffer(s, np.uint8).copy()).cuda()
        cap = int(lib.lz4flex_frame_segment_bound(SIZE, C.byref(fic))) + 64
        frame, out = torch.zeros(cap, dtype=torch.uint8, device="cuda"), torch.zeros(3 * BS, dtype=torch.uint8, device="cuda")
        flen, olen, first, nblk = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        torch.cuda.synchronize()
        assert lib.lz4flex_frame_compress_sharded(ctx, None, 0, 1, 0, C.c_void_p(src.data_ptr()), SIZE, 0, C.byref(fic), C.c_void_p(frame.data_ptr()),
                                                  cap, C.byref(flen), None) == 0, L.last_error()
        assert lib.lz4flex_frame_decompress_sharded(ctx, None, 0, 1, 0, C.c_void_p(frame.data_ptr()), flen.value, C.c_void_p(out.data_ptr()),
                                                    int(out.numel()), C.byref(olen), C.byref(first), C.byref(nblk), None, None, None) == 0, L.last_error()
        assert (olen.value, first.value, nblk.value) == (SIZE, 0, 3) and out[:SIZE].cpu().numpy().tobytes() == s
    lib.lz4flex_ctx_destroy(ctx)
    print("frame_calls_trace: ok")


def run_stream():
    import io
    import oracle_api as O
    from lz4_flex_amd import block, frame as F
    text = O.fixture_plain("compression_65k") + O.fixture_plain("compression_66k_JSON")
    linked_chunks = [BS, BS, BS, 1000, BS, 30000, BS, BS]
    for mode, chunks in ((1, linked_chunks), (0, [5 * BS + 1000])):
        n = sum(chunks)
        data = (text * (n // len(text) + 1))[:n]
        info = F.FrameInfo(block_mode=F.BlockMode(mode), block_size=F.BlockSize.Max64KB)
        for cm in ("fast", "exact"):
            block.set_compress_mode(cm)
            try:
                buf, at = io.BytesIO(), 0
                e = F.FrameEncoder.with_frame_info(info, buf)
                for c in chunks:
                    e.write(data[at:at + c]); e.flush()
                    at += c
                e.finish()
                one = F.compress_frame(data, info)
            finally:
                block.set_compress_mode("fast")
            for f in (buf.getvalue(), one):
                assert O.frame_decompress(f, n) == (0, data, len(f))
            for size in (BS, 1 << 20):
                d, out = F.FrameDecoder.new(io.BytesIO(buf.getvalue())), []
                while True:
                    b = d.read(size)
                    if not b:
                        break
                    out.append(b)
                assert b"".join(out) == data
            assert F.decompress_frame(one, n) == (data, len(one))
    print("frame_calls_trace: stream ok")


def short(name):
    name = re.sub(r"\s*\[clone .*$", "", name)
    return re.sub(r"^void\s+", "", re.sub(r"\(.*$", "", name)).strip()


def listing(tdir):
    rows = []
    for path in sorted(glob.glob(os.path.join(tdir, "**", "*.json"), recursive=True)):
        with open(path) as f:
            doc = json.load(f)
        for proc in doc.get("rocprofiler-sdk-tool", []):
            names = {k["kernel_id"]: k.get("formatted_kernel_name") or k.get("demangled_kernel_name") or k.get("kernel_name")
                     for k in proc.get("kernel_symbols", [])}
            ops = {}
            for kind in proc.get("strings", {}).get("buffer_records", []):
                if kind.get("kind") == "MEMORY_COPY":
                    ops = dict(enumerate(kind.get("operations", [])))
            rec = proc.get("buffer_records", {})
            for k in rec.get("kernel_dispatch", []):
                rows.append((k["start_timestamp"], "K %s" % short(names.get(k["dispatch_info"]["kernel_id"], "?"))))
            for m in rec.get("memory_copy", []):
                op = ops.get(m.get("operation"), str(m.get("operation"))).replace("MEMORY_COPY_", "")
                rows.append((m["start_timestamp"], "C %s %d" % (op, m.get("bytes", -1))))
    for _, line in sorted(rows, key=lambda r: r[0]):
        print(line)


def copies(log):
    pat = re.compile(r"(hipMemcpy\w*) \( [^,]+, [^,]+, (\d+), (hipMemcpy\w+)")
    with open(log, errors="replace") as f:
        for line in f:
            m = pat.search(line)
            if m:
                print("M %s %s %s" % (m.group(1), m.group(3).replace("hipMemcpy", ""), m.group(2)))


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) >= 2 and sys.argv[1] == "run-stream":
        run_stream()
    elif len(sys.argv) == 3 and sys.argv[1] == "list":
        listing(sys.argv[2])
    elif len(sys.argv) == 3 and sys.argv[1] == "copies":
        copies(sys.argv[2])
    else:
        sys.exit(__doc__)
