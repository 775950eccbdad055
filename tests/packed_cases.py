"""What the GPU tests of the packed batch entries share (tests/test_gpu_packed_decode.py, tests/test_gpu_packed_compress.py): the calls
through the C ABI in both memory kinds with canaries around everything that is written, and the expected layout -- numpy's cumsum of
the sizes rounded up to `align`, in uint64 -- with the fit rule.  A plain module, not a fixture."""
import ctypes as C

import numpy as np

import oracle_api as O

CANARY = 0xC5
TAIL = 512                      # canary bytes behind the buffer's capacity
CODES = {v: k for k, v in O.ERR_NAMES.items()}
E_OUTPUT_TOO_SMALL, E_EXPECTED_ANOTHER_BYTE, E_UNSUPPORTED = 1, 3, 68


def le32(v):
    return int(v).to_bytes(4, "little")


def pack(blocks, odd=False):
    """blocks laid out one behind the other (odd: every block starts at an odd offset, with a gap in front): (buf, off, len)"""
    offs, lens, at = [], [], 0
    for c in blocks:
        if odd:
            at += 2 if at & 1 else 1                            # the next odd offset behind at least one byte of gap
        offs.append(at)
        lens.append(len(c))
        at += len(c)
    buf = bytearray(max(at, 1) + 8)
    for o, c in zip(offs, blocks):
        buf[o:o + len(c)] = c
    if odd:
        assert all(o & 1 for o in offs)
    return np.frombuffer(bytes(buf), np.uint8), np.array(offs, np.uint64), np.array(lens, np.uint32)


def layout(sizes, align):
    """out_off[0 .. n] as the issue defines it: cumsum of the sizes rounded up to align, uint64"""
    sizes = np.asarray(sizes, np.uint64)
    a = np.uint64(align)
    rounded = (sizes + (a - np.uint64(1))) // a * a
    off = np.zeros(len(sizes) + 1, np.uint64)
    np.cumsum(rounded, dtype=np.uint64, out=off[1:])
    return off


def _dev(a):
    import torch
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))


def _host(t, dt):
    return t.cpu().numpy().view(dt)


def decode(lib, ctx, buf, offs, lens, mode, sizes, align, total_cap, room, mem="device", big=False):
    """lz4flex_decompress_batch_packed; the output buffer has `room` + TAIL bytes (>= total_cap), all canary before the call.
    Returns dict(out_off, out_cap, out_len, status, detail, out)."""
    from lz4_flex_amd import _lib
    n = len(offs)
    assert room >= total_cap
    flags = _lib.MEM_BIG_BLOCKS if big else 0
    r = dict(out_off=np.full(n + 2, 0xA5A5A5A5A5A5A5A5, np.uint64), out_cap=np.full(n + 1, 0xA5A5A5A5, np.uint32),
             out_len=np.full(n + 1, 0xA5A5A5A5, np.uint32), status=np.full(n + 1, 0x5A5A5A5A, np.int32),
             detail=np.full(2 * n + 2, 0xA5A5A5A5A5A5A5A5, np.uint64), out=np.full(room + TAIL, CANARY, np.uint8))
    sz = None if sizes is None else np.ascontiguousarray(sizes, np.uint32)
    if mem == "host":
        p = lambda a: C.c_void_p(a.ctypes.data)
        rc = lib.lz4flex_decompress_batch_packed(ctx, p(buf), p(offs), p(lens), n, mode, None if sz is None else p(sz), p(r["out"]), total_cap,
                                                 align, p(r["out_off"]), p(r["out_cap"]), p(r["out_len"]), p(r["status"]), p(r["detail"]), None,
                                                 _lib.MEM_HOST | flags, None)
        assert rc == 0, (rc, _lib.last_error())
    else:
        import torch
        t = {k: _dev(v) for k, v in r.items()}
        d_buf, d_offs, d_lens = _dev(buf), _dev(offs), _dev(lens)
        d_sz = None if sz is None else _dev(sz)
        work = torch.empty(int(lib.lz4flex_packed_work_size(n)) + 64, dtype=torch.uint8, device=d_buf.device)
        stream = torch.cuda.current_stream(d_buf.device)
        p = lambda x: C.c_void_p(x.data_ptr())
        rc = lib.lz4flex_decompress_batch_packed(ctx, p(d_buf), p(d_offs), p(d_lens), n, mode, None if d_sz is None else p(d_sz), p(t["out"]),
                                                 total_cap, align, p(t["out_off"]), p(t["out_cap"]), p(t["out_len"]), p(t["status"]),
                                                 p(t["detail"]), p(work), _lib.MEM_DEVICE | flags, C.c_void_p(stream.cuda_stream))
        assert rc == 0, (rc, _lib.last_error())
        stream.synchronize()
        r = {k: _host(t[k], v.dtype) for k, v in r.items()}
    assert r["out_off"][n + 1] == 0xA5A5A5A5A5A5A5A5 and r["out_cap"][n] == 0xA5A5A5A5 and r["out_len"][n] == 0xA5A5A5A5
    assert r["status"][n] == 0x5A5A5A5A and (r["detail"][2 * n:] == 0xA5A5A5A5A5A5A5A5).all(), "results written past n"
    return dict(out_off=r["out_off"][:n + 1], out_cap=r["out_cap"][:n], out_len=r["out_len"][:n], status=r["status"][:n],
                detail=r["detail"][:2 * n].reshape(n, 2), out=r["out"])


def compress(lib, ctx, buf, offs, lens, prepend, align, total_cap, room, mem="device", big=False, scratch_cap=None):
    """lz4flex_compress_batch_packed, canaries as in decode().  Returns dict(out_off, out_len, status, out)."""
    from lz4_flex_amd import _lib
    n = len(offs)
    flags = _lib.MEM_BIG_BLOCKS if big else 0
    bound = int(lib.lz4flex_compress_packed_scratch_bound(int(lens.sum(dtype=np.uint64)), n, prepend))
    scratch_cap = bound if scratch_cap is None else scratch_cap
    r = dict(out_off=np.full(n + 2, 0xA5A5A5A5A5A5A5A5, np.uint64), out_len=np.full(n + 1, 0xA5A5A5A5, np.uint32),
             status=np.full(n + 1, 0x5A5A5A5A, np.int32), out=np.full(room + TAIL, CANARY, np.uint8))
    if mem == "host":
        p = lambda a: C.c_void_p(a.ctypes.data)
        rc = lib.lz4flex_compress_batch_packed(ctx, p(buf), p(offs), p(lens), n, prepend, None, scratch_cap, p(r["out"]), total_cap, align,
                                               p(r["out_off"]), p(r["out_len"]), p(r["status"]), None, _lib.MEM_HOST | flags, None)
        assert rc == 0, (rc, _lib.last_error())
    else:
        import torch
        t = {k: _dev(v) for k, v in r.items()}
        d_buf, d_offs, d_lens = _dev(buf), _dev(offs), _dev(lens)
        work = torch.empty(int(lib.lz4flex_packed_work_size(n)) + 64, dtype=torch.uint8, device=d_buf.device)
        scratch = torch.full((max(scratch_cap, 1) + TAIL,), CANARY, dtype=torch.uint8, device=d_buf.device)
        stream = torch.cuda.current_stream(d_buf.device)
        p = lambda x: C.c_void_p(x.data_ptr())
        rc = lib.lz4flex_compress_batch_packed(ctx, p(d_buf), p(d_offs), p(d_lens), n, prepend, p(scratch), scratch_cap, p(t["out"]), total_cap,
                                               align, p(t["out_off"]), p(t["out_len"]), p(t["status"]), p(work), _lib.MEM_DEVICE | flags,
                                               C.c_void_p(stream.cuda_stream))
        assert rc == 0, (rc, _lib.last_error())
        stream.synchronize()
        assert bool((scratch[scratch_cap:] == CANARY).all()), "written behind scratch_cap"
        r = {k: _host(t[k], v.dtype) for k, v in r.items()}
    assert r["out_off"][n + 1] == 0xA5A5A5A5A5A5A5A5 and r["out_len"][n] == 0xA5A5A5A5 and r["status"][n] == 0x5A5A5A5A, "results written past n"
    return dict(out_off=r["out_off"][:n + 1], out_len=r["out_len"][:n], status=r["status"][:n], out=r["out"])


def oracle_block(raw, size):
    """(status, out_len, detail, bytes) of decompress_into(raw, a sink of `size` bytes) by the oracle"""
    st, res = O.decompress(raw, int(size))
    if st == "ok":
        return 0, len(res), (0, 0), res
    return CODES[st], 0, (res if st == "OutputTooSmall" else (0, 0)), b""


def expect_decode(results, sizes, pre, align, total_cap):
    """results: oracle_block per block (ignored where pre[i] != 0: a block without a size); the expected arrays under the fit rule"""
    n = len(sizes)
    off = layout(sizes, align)
    out_cap, out_len, status = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.int32)
    detail = np.zeros((n, 2), np.uint64)
    pieces = []
    for i in range(n):
        end = int(off[i]) + int(sizes[i])
        if end > total_cap:
            status[i] = E_OUTPUT_TOO_SMALL
            detail[i] = (end, total_cap)
        elif pre[i]:
            status[i] = pre[i]
        else:
            st, ln, det, data = results[i]
            out_cap[i], out_len[i], status[i], detail[i] = sizes[i], ln, st, det
            pieces.append((int(off[i]), data, st != 0, int(sizes[i])))
    return dict(out_off=off, out_cap=out_cap, out_len=out_len, status=status, detail=detail, pieces=pieces)


def check_decode(got, want, what=""):
    for k in ("out_off", "out_cap", "out_len", "status", "detail"):
        bad = np.nonzero((got[k] != want[k]).reshape(len(got[k]), -1).any(axis=1))[0]
        assert bad.size == 0, "%s %s: %d entries differ, first %d: got %s, want %s" % (what, k, bad.size, bad[0], got[k][bad[0]], want[k][bad[0]])
    image = np.full(got["out"].size, CANARY, np.uint8)
    for at, data, failed, slot in want["pieces"]:
        if failed:
            # a block the decoder gave up on may have left what it had decoded so far in its own slot, as decompress_into does in its
            # sink (lz4flex_decompress_batch: the same); nothing outside the slot
            image[at:at + slot] = got["out"][at:at + slot]
        else:
            image[at:at + len(data)] = np.frombuffer(data, np.uint8)
    bad = np.nonzero(got["out"] != image)[0]
    assert bad.size == 0, "%s: %d output bytes differ from the oracle / the canary, first at %d" % (what, bad.size, bad[0])
