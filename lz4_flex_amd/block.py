"""lz4_flex::block, MI355X edition (reference src/block/{compress,decompress,mod}.rs).

Same names, argument meaning and error behaviour as the reference's public block API; every call
runs the HIP kernels through the C ABI.  Errors are exceptions named after the Rust enum variants
(src/block/mod.rs:82-106)."""
import ctypes as C

import numpy as np

from . import _lib as L


class CompressError(Exception):
    """block::CompressError (mod.rs:103-106)"""


class CompressOutputTooSmall(CompressError):
    pass


class DecompressError(Exception):
    """block::DecompressError (mod.rs:82-98)"""


class OutputTooSmall(DecompressError):
    def __init__(self, expected, actual):
        super().__init__("provided output is too small for the decompressed data, actual %d, expected %d"
                         % (actual, expected))
        self.expected, self.actual = expected, actual


class LiteralOutOfBounds(DecompressError):
    pass


class ExpectedAnotherByte(DecompressError):
    pass


class OffsetZero(DecompressError):
    pass


class OffsetOutOfBounds(DecompressError):
    pass


class DeviceError(RuntimeError):
    """HIP/runtime failure or an entry point whose GPU path is not built (no CPU fallback exists)."""


_DECODE_ERRORS = {L.E_LITERAL_OUT_OF_BOUNDS: LiteralOutOfBounds, L.E_EXPECTED_ANOTHER_BYTE: ExpectedAnotherByte,
                  L.E_OFFSET_ZERO: OffsetZero, L.E_OFFSET_OUT_OF_BOUNDS: OffsetOutOfBounds}


def _raise_decode(code, detail):
    if code == L.E_OUTPUT_TOO_SMALL:
        raise OutputTooSmall(detail.expected, detail.actual)
    if code in _DECODE_ERRORS:
        raise _DECODE_ERRORS[code]()
    raise DeviceError("lz4flex error %d: %s" % (code, L.last_error()))


def _check(rc, name):
    """the return code of the C entry `name`"""
    if rc:
        raise DeviceError("%s failed (%d): %s" % (name, rc, L.last_error()))


def _buf(b):
    """bytes-like -> (ctypes pointer, length, keepalive)"""
    if isinstance(b, (bytes, bytearray)):
        arr = (C.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) if len(b) else b"\0")
        return C.cast(arr, C.c_void_p), len(b), arr
    a = np.ascontiguousarray(np.frombuffer(memoryview(b), dtype=np.uint8))
    return C.c_void_p(a.ctypes.data if a.size else 0), int(a.size), a


def set_compress_mode(mode, ctx=None):
    """Encoder of this thread's default context (or of `ctx`): "fast" = throughput encoder (own parse: a valid LZ4 block
    that lz4_flex decodes to the input; default), "exact" = lz4_flex's own bytes (src/block/compress.rs:318-489), "high" = a deep
    search for smaller blocks (set_compress_depth candidates per position; independent blocks -- Linked frames get "fast"'s bytes unless
    set_compress_high_linked(True), and so do dictionary calls unless set_compress_high_dict(True))."""
    v = {"fast": 0, "exact": 1, "high": 2}[mode]
    _check(L.load().lz4flex_set_tuning(ctx, b"compress_mode", v), "lz4flex_set_tuning(compress_mode)")


def set_compress_depth(depth, ctx=None):
    """"compress_depth" of this thread's default context (or of `ctx`): the candidates compress mode "high" examines per position,
    1 .. 256 (default 16).  The other modes do not read it."""
    _check(L.load().lz4flex_set_tuning(ctx, b"compress_depth", int(depth)), "lz4flex_set_tuning(compress_depth)")


def set_compress_parse(parse, ctx=None):
    """"compress_parse" of this thread's default context (or of `ctx`): how compress mode "high" turns its matches into sequences.
    "lazy" (default) takes a position's longest match whole unless the next position has a longer one; "optimal" prices every position
    backwards and may take a part of the match (tests/sim/high_optimal_model.c) -- 1.6 % to 3.4 % smaller blocks on text, JSON and logs
    at every depth, some more encode time.  An unknown name raises KeyError.  The other modes do not read it."""
    v = {"lazy": 0, "optimal": 1}[parse]
    _check(L.load().lz4flex_set_tuning(ctx, b"compress_parse", v), "lz4flex_set_tuning(compress_parse)")


def set_compress_high_dict(on, ctx=None):
    """"compress_high_dict" of this thread's default context (or of `ctx`): with compress mode "high", True makes every call that
    takes dictionaries (compress_with_dict, compress_prepend_size_with_dict, compress_batch_with_dict, _with_shared_dict,
    _with_dict_set) search the dictionary's last 32 KiB as deeply as the block itself -- smaller blocks that every dictionary decoder
    here reads; False (default): those calls give "fast"'s bytes.  The other modes do not read it."""
    _check(L.load().lz4flex_set_tuning(ctx, b"compress_high_dict", 1 if on else 0), "lz4flex_set_tuning(compress_high_dict)")


def set_compress_high_linked(on, ctx=None):
    """"compress_high_linked" of this thread's default context (or of `ctx`): with compress mode "high", True makes a Linked frame's
    blocks (and every batch block whose flag word carries LZ4FLEX_BLOCK_HISTORY bits) search the up to 32 KiB of their stream in
    front of them as deeply as the block itself -- smaller frames that every LZ4 frame decoder reads; False (default): Linked frames
    give "fast"'s bytes and the history bits are ignored.  The other modes do not read it."""
    _check(L.load().lz4flex_set_tuning(ctx, b"compress_high_linked", 1 if on else 0), "lz4flex_set_tuning(compress_high_linked)")


def get_maximum_output_size(input_len):
    """block::get_maximum_output_size (compress.rs:588-590)"""
    return int(L.load().lz4flex_get_maximum_output_size(int(input_len)))


def compress_into(input, output):
    """block::compress_into (compress.rs:599-601): `output` is a writable buffer; returns bytes written."""
    lib = L.load()
    ip, n, _k = _buf(input)
    out = (C.c_uint8 * max(len(output), 1)).from_buffer(output) if len(output) else (C.c_uint8 * 1)()
    r = lib.lz4flex_compress_into(ip, n, C.cast(out, C.c_void_p), len(output))
    if r == -L.E_OUTPUT_TOO_SMALL:
        raise CompressOutputTooSmall("output is too small for the compressed data, use get_maximum_output_size "
                                     "to reserve enough space")
    if r < 0:
        raise DeviceError("lz4flex error %d: %s" % (-r, L.last_error()))
    return int(r)


def compress(input):
    """block::compress (compress.rs:679-681)"""
    out = bytearray(get_maximum_output_size(len(input)))
    n = compress_into(input, out)
    return bytes(out[:n])


def compress_prepend_size(input):
    """block::compress_prepend_size (compress.rs:673-675)"""
    return len(input).to_bytes(4, "little") + compress(input)


class CompressTable:
    """block::CompressTable (compress.rs:710-740): small() / large() / default; reused across compress_into_with_table calls"""

    def __init__(self, large=False):
        self._h = L.load().lz4flex_compress_table_new(1 if large else 0)
        if not self._h:
            raise DeviceError("lz4flex_compress_table_new failed: " + L.last_error())

    @classmethod
    def small(cls):
        return cls(False)

    @classmethod
    def large(cls):
        return cls(True)

    @property
    def is_large(self):
        return bool(L.load().lz4flex_compress_table_is_large(self._h))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                L.load().lz4flex_compress_table_free(h)
            except Exception:
                pass


def compress_into_with_table(input, output, table):
    """block::compress_into_with_table (compress.rs:742-766)"""
    lib = L.load()
    ip, n, _k = _buf(input)
    out = (C.c_uint8 * max(len(output), 1)).from_buffer(output) if len(output) else (C.c_uint8 * 1)()
    r = lib.lz4flex_compress_into_with_table(ip, n, C.cast(out, C.c_void_p), len(output), table._h)
    if r == -L.E_OUTPUT_TOO_SMALL:
        raise CompressOutputTooSmall()
    if r < 0:
        raise DeviceError("lz4flex error %d: %s" % (-r, L.last_error()))
    return int(r)


def compress_prepend_size_with_dict(input, ext_dict):
    """block::compress_prepend_size_with_dict (compress.rs:692-694), through the C entry point"""
    lib = L.load()
    ip, n, _k = _buf(input)
    dp, dn, _k2 = _buf(ext_dict)
    out = bytearray(4 + get_maximum_output_size(n))
    o = (C.c_uint8 * len(out)).from_buffer(out)
    r = lib.lz4flex_compress_prepend_size_with_dict(ip, n, C.cast(o, C.c_void_p), len(out), dp, dn)
    if r < 0:
        raise DeviceError("lz4flex error %d: %s" % (-r, L.last_error()))
    del o
    return bytes(out[:r])


def compress_into_with_dict(input, output, dict_data):
    """block::compress_into_with_dict (compress.rs:610-616)"""
    lib = L.load()
    ip, n, _k = _buf(input)
    dp, dn, _k2 = _buf(dict_data)
    out = (C.c_uint8 * max(len(output), 1)).from_buffer(output) if len(output) else (C.c_uint8 * 1)()
    r = lib.lz4flex_compress_into_with_dict(ip, n, C.cast(out, C.c_void_p), len(output), dp, dn)
    if r == -L.E_OUTPUT_TOO_SMALL:
        raise CompressOutputTooSmall()
    if r < 0:
        raise DeviceError("lz4flex error %d: %s" % (-r, L.last_error()))
    return int(r)


def compress_with_dict(input, ext_dict):
    """block::compress_with_dict (compress.rs:685-687); dicts of <= 3 bytes are ignored (:626-628)"""
    if len(ext_dict) <= 3:
        return compress(input)
    out = bytearray(get_maximum_output_size(len(input)))
    n = compress_into_with_dict(input, out, ext_dict)
    return bytes(out[:n])


def decompress_into(input, output):
    """block::decompress_into (decompress.rs:454-456): returns bytes written."""
    lib = L.load()
    ip, n, _k = _buf(input)
    out = (C.c_uint8 * max(len(output), 1)).from_buffer(output) if len(output) else (C.c_uint8 * 1)()
    d = L.ErrDetail()
    r = lib.lz4flex_decompress_into(ip, n, C.cast(out, C.c_void_p), len(output), C.byref(d))
    if r < 0:
        _raise_decode(int(-r), d)
    return int(r)


def decompress_into_with_dict(input, output, ext_dict):
    """block::decompress_into_with_dict (decompress.rs:462-468)"""
    lib = L.load()
    ip, n, _k = _buf(input)
    dp, dn, _k2 = _buf(ext_dict)
    out = (C.c_uint8 * max(len(output), 1)).from_buffer(output) if len(output) else (C.c_uint8 * 1)()
    d = L.ErrDetail()
    r = lib.lz4flex_decompress_into_with_dict(ip, n, C.cast(out, C.c_void_p), len(output), dp, dn, C.byref(d))
    if r < 0:
        _raise_decode(int(-r), d)
    return int(r)


def decompress(input, min_uncompressed_size):
    """block::decompress (decompress.rs:506-517)"""
    out = bytearray(min_uncompressed_size)
    n = decompress_into(input, out)
    return bytes(out[:n])


def decompress_with_dict(input, min_uncompressed_size, ext_dict):
    """block::decompress_with_dict (decompress.rs:478-489)"""
    out = bytearray(min_uncompressed_size)
    n = decompress_into_with_dict(input, out, ext_dict)
    return bytes(out[:n])


def decompress_partial(input, n):
    """The first min(size, n) bytes of the block `input` (lz4flex_decompress_partial_into: liblz4's LZ4_decompress_safe_partial).  An
    error the reference would meet before n bytes exist is raised as block::decompress raises it; one behind that point is not seen,
    and there is no OutputTooSmall."""
    lib = L.load()
    ip, ilen, _k = _buf(input)
    out = bytearray(max(int(n), 1))
    o = (C.c_uint8 * len(out)).from_buffer(out)
    d = L.ErrDetail()
    r = lib.lz4flex_decompress_partial_into(ip, ilen, C.cast(o, C.c_void_p), int(n), C.byref(d))
    del o
    if r < 0:
        _raise_decode(int(-r), d)
    return bytes(out[:r])


def decompress_partial_with_dict(input, n, ext_dict):
    """The first min(size, n) bytes of the block `input`, which was compressed against `ext_dict` (lz4flex_decompress_partial_into_with_dict):
    decompress_partial with block::decompress_with_dict's offset rule -- an offset may reach len(ext_dict) bytes in front of the output."""
    lib = L.load()
    ip, ilen, _k = _buf(input)
    dp, dn, _k2 = _buf(ext_dict)
    out = bytearray(max(int(n), 1))
    o = (C.c_uint8 * len(out)).from_buffer(out)
    d = L.ErrDetail()
    r = lib.lz4flex_decompress_partial_into_with_dict(ip, ilen, C.cast(o, C.c_void_p), int(n), dp, dn, C.byref(d))
    del o
    if r < 0:
        _raise_decode(int(-r), d)
    return bytes(out[:r])


def uncompressed_size(input):
    """block::uncompressed_size (mod.rs:151-157): (size, rest)"""
    if len(input) < 4:
        raise ExpectedAnotherByte()
    return int.from_bytes(bytes(input[:4]), "little"), input[4:]


def decompress_size_prepended(input):
    """block::decompress_size_prepended (decompress.rs:493-496)"""
    size, rest = uncompressed_size(input)
    return decompress(rest, size)


def decompress_size_prepended_with_dict(input, ext_dict):
    """block::decompress_size_prepended_with_dict (decompress.rs:521-527), through the C entry point"""
    lib = L.load()
    size, _rest = uncompressed_size(input)
    ip, n, _k = _buf(input)
    dp, dn, _k2 = _buf(ext_dict)
    out = bytearray(max(size, 1))
    o = (C.c_uint8 * len(out)).from_buffer(out)
    d = L.ErrDetail()
    r = lib.lz4flex_decompress_size_prepended_with_dict(ip, n, C.cast(o, C.c_void_p), size, dp, dn, C.byref(d))
    del o
    if r < 0:
        _raise_decode(int(-r), d)
    return bytes(out[:r])


# ---- batched entry points -------------------------------------------------------------------------
# Every batched entry of the C ABI has one shape:
#     name(ctx, in_base, in_off, in_len, [flags,] n, <what is particular to it>, out_len, status, [detail,] <more of that>, mem_kind, stream)
# The host forms (numpy arrays in, numpy arrays out) are one _host_call each; the device forms (torch tensors) share _device_args and
# _device_call, the three that compress into slots of the maximum output size _compress_slots_device, the three that decode blocks of
# unknown sizes _size_then_decode_device, the three that decode up to a target _partial_device.  A form keeps its docstring, what is particular to it, and its return.
NO_DICT = 0xFFFFFFFF     # the dict_id of a block without a dictionary (lz4flex_dict_set_*, lz4flex_*_batch_dict_set)
SIZE_MODES = {"prepended": L.SIZES_PREPENDED, "given": L.SIZES_GIVEN, "scan": L.SIZES_SCAN}     # lz4flex_decompress_batch_packed


def _host_u8(b):
    return b if isinstance(b, np.ndarray) else np.ascontiguousarray(np.frombuffer(memoryview(b), dtype=np.uint8))


def _np(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _u32(a):
    return None if a is None else _np(a, np.uint32)


def _arg(a):
    """one argument as ctypes takes it: a numpy array or a torch tensor by its address (NULL when it is empty), a DictSet by its handle,
    anything else as it is"""
    if isinstance(a, np.ndarray):
        return C.c_void_p(a.ctypes.data) if a.size else None
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr()) if a.numel() else None
    return a.handle if isinstance(a, DictSet) else a


def _host_call(name, ctx, in_buf, in_off, in_len, out=None, before_n=(), middle=(), tail=(), detail=False, len_dtype=np.uint32,
               mem_kind=L.MEM_HOST, per_call=False, results=True, in_used=False):
    """The host marshaller:
        name(ctx, in_base, in_off, in_len, *before_n, n, *middle, [out_base, out_off, out_cap,] out_len, [in_used,] status, [detail,] *tail, mem_kind, NULL)
    in_buf is bytes-like or a uint8 array, in_off / in_len and `out` = (out_buf, out_off, out_cap) anything numpy converts; before_n,
    middle and tail hold what is particular to the entry, each as _arg takes it.  Returns the arrays the call wrote: (out_len[len_dtype],
    status[i32]) and, with `detail`, detail[n, 2] u64; per_call: the entry writes ONE length and ONE status for the whole batch; results
    False: the entry has neither (lz4flex_filter_batch), () is returned; in_used: the fit entries' in_used[u32] between the two."""
    n = len(in_off)
    m = 1 if per_call else n
    results = [] if not results else \
        [np.zeros(m, dtype=len_dtype)] + ([np.zeros(m, dtype=np.uint32)] if in_used else []) + [np.zeros(m, dtype=np.int32)] + \
        ([np.zeros((n, 2), dtype=np.uint64)] if detail else [])
    slots = [] if out is None else [out[0], _np(out[1], np.uint64), _np(out[2], np.uint32)]
    args = [_host_u8(in_buf), _np(in_off, np.uint64), _np(in_len, np.uint32), *before_n, n, *middle, *slots, *results, *tail]
    _check(getattr(L.load(), name)(ctx, *map(_arg, args), mem_kind, None), name)
    return tuple(results)


def _host_dict_ext(ext_type, dict_buf, dict_off, dict_len):
    """the ext structure of per-block dictionaries, and the arrays it points into (to keep until the call returns)"""
    keep = [_host_u8(dict_buf), _np(dict_off, np.uint64), _np(dict_len, np.uint32)]
    if not keep[0].size:
        keep[0] = np.zeros(1, dtype=np.uint8)     # (an empty dictionary buffer still needs an address: NULL would mean "no dictionaries")
    return ext_type(*(a.ctypes.data if a.size else None for a in keep)), keep


def _host_ids(dict_id, n):
    ids = _np(dict_id, np.uint32)
    if len(ids) != n:
        raise ValueError("in_off and dict_id differ in length")
    return ids


def _device_args(src, in_off, in_len, stream, wide_len=False, **companions):
    """The device prologue: src (and every companion, by its parameter's name) is a contiguous uint8 tensor on one GPU, in_off / in_len
    have one length.  Returns (device, n, in_off as int64, in_len as int32 -- wide_len: int64 --, the stream's pointer; default: the
    current stream)."""
    import torch
    dev = src.device
    if dev.type != "cuda" or src.dtype != torch.uint8 or not src.is_contiguous():
        raise ValueError("src must be a contiguous uint8 tensor on the GPU")
    for name, t in companions.items():
        if t.device != dev or t.dtype != torch.uint8 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous uint8 tensor on the GPU of src" % name)
    n = int(in_off.numel())
    if int(in_len.numel()) != n:
        raise ValueError("in_off and in_len differ in length")
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    return (dev, n, in_off.to(device=dev, dtype=torch.int64).contiguous(),
            in_len.to(device=dev, dtype=torch.int64 if wide_len else torch.int32).contiguous(), C.c_void_p(stream))


def _device_call(name, head, n, rest, big_blocks, stream_ptr, ctx=None):
    """name(ctx, *head, n, *rest, MEM_DEVICE [| MEM_BIG_BLOCKS], stream), every argument as _arg takes it"""
    mem_kind = L.MEM_DEVICE | (L.MEM_BIG_BLOCKS if big_blocks else 0)
    _check(getattr(L.load(), name)(ctx, *map(_arg, head), n, *map(_arg, rest), mem_kind, stream_ptr), name)


def _compress_slots_device(name, src, in_off, in_len, stream, before_n=(), after_n=(), tail=(), **companions):
    """The device compress recipe: one
        name(NULL, src, in_off, in_len, *before_n, n, *after_n, out, out_off, out_cap, out_len, status, *tail, mem_kind, stream)
    into slots of get_maximum_output_size(in_len[i]) bytes, asynchronous on `stream`.  Returns (out, out_off, out_len, status)."""
    import torch
    dev, n, d_off, d_len, sp = _device_args(src, in_off, in_len, stream, wide_len=True, **companions)
    cap64 = 20 + d_len * 110 // 100                      # get_maximum_output_size, compress.rs:588-590
    out_off = torch.cumsum(cap64, 0) - cap64
    total = int(cap64.sum()) if n else 0
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    out_len = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    if n == 0:
        return out[:0], out_off, out_len, status
    _device_call(name, [src, d_off, d_len.to(torch.int32), *before_n], n, [*after_n, out, out_off, cap64.to(torch.int32), out_len, status, *tail],
                 int(d_len.max()) > 65536, sp)
    return out[:total], out_off, out_len, status


def _size_then_decode_device(name, src, in_off, in_len, stream, history=None, after_n=(), tail=(), decoder_wins=None, **companions):
    """The device decode recipe for raw blocks of unknown sizes: the size pass (history: an int32 tensor of the bytes in front of each
    block, or None), an exclusive prefix sum for the output offsets, ONE host synchronisation (the total, to allocate exactly that), one
        name(NULL, src, in_off, in_len, n, *after_n, out, out_off, out_cap = the sizes, out_len, status, NULL, *tail, mem_kind, stream)
    A block the size pass rejected keeps that status, unless the decoder's is `decoder_wins`; a block that fails has an empty slot.
    Returns (out, out_off, out_len, status)."""
    import torch
    dev, n, d_off, d_len, sp = _device_args(src, in_off, in_len, stream, **companions)
    size = torch.empty(n, dtype=torch.int64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return torch.empty(0, dtype=torch.uint8, device=dev), size, torch.empty(0, dtype=torch.int32, device=dev), status
    _device_call("lz4flex_decompressed_size_batch", [src, d_off, d_len], n, [history, size, status], False, sp)
    incl = torch.cumsum(size, 0)
    out_off = incl - size
    total, biggest = (int(v) for v in torch.stack([incl[-1], size.max()]).cpu())     # the one synchronisation
    if biggest > 0xFFFFFFFF:
        raise ValueError("a block decompresses to %d bytes: more than the decoders' u32 out_cap" % biggest)
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    cap = size.to(torch.int32)       # (the bit pattern of a u32 <= 0xFFFFFFFF)
    out_len = torch.zeros(n, dtype=torch.int32, device=dev)
    st2 = torch.empty(n, dtype=torch.int32, device=dev)
    _device_call(name, [src, d_off, d_len], n, [*after_n, out, out_off, cap, out_len, st2, None, *tail], biggest > 131072, sp)
    # (the decoder's status is the one of every block the size pass accepted: 0 by the size pass's contract)
    rejected = status != 0 if decoder_wins is None else (status != 0) & (st2 != decoder_wins)
    status = torch.where(rejected, status, st2)
    out_len = torch.where(status != 0, torch.zeros_like(out_len), out_len)
    return out[:total], out_off, out_len, status


# ---- plain batches ------------------------------------------------------------------------------------------------------------
def compress_batch(in_buf, in_off, in_len, out_buf, out_off, out_cap, flags=None, ctx=None):
    """lz4flex_compress_batch over host buffers: returns (out_len[u32], status[i32])."""
    return _host_call("lz4flex_compress_batch", ctx, in_buf, in_off, in_len, (out_buf, out_off, out_cap), before_n=[_u32(flags)])


def decompress_batch(in_buf, in_off, in_len, out_buf, out_off, out_cap, ctx=None):
    """lz4flex_decompress_batch over host buffers: returns (out_len[u32], status[i32], detail[n,2] u64)."""
    return _host_call("lz4flex_decompress_batch", ctx, in_buf, in_off, in_len, (out_buf, out_off, out_cap), detail=True)


def decompressed_size_batch(in_buf, in_off, in_len, history=None, ctx=None):
    """lz4flex_decompressed_size_batch over host buffers: for raw blocks without their sizes, (size[u64], status[i32]) -- the bytes
    decompress_into would produce with an unbounded sink and history[i] (None: 0) bytes in front of the block, or its error code (size
    0).  Nothing is decoded."""
    return _host_call("lz4flex_decompressed_size_batch", ctx, in_buf, in_off, in_len, middle=[_u32(history)], len_dtype=np.uint64)


def decompress_blocks_device(src, in_off, in_len, stream=None):
    """Raw blocks in device memory, sizes unknown: src is a uint8 torch tensor on the GPU, in_off / in_len integer tensors (block i is
    src[in_off[i] : in_off[i] + in_len[i]]).  The size pass, an exclusive prefix sum for the output offsets, ONE host synchronisation (the
    total, to allocate exactly that), one lz4flex_decompress_batch with out_cap = the sizes.  Returns (out, out_off, out_len, status) as
    device tensors: block i's bytes are out[out_off[i] : out_off[i] + out_len[i]]; a block that fails gets its status and an empty slot.
    A block of more than 4 GiB - 1 decompressed bytes (the decoders' u32 out_cap) raises ValueError."""
    return _size_then_decode_device("lz4flex_decompress_batch", src, in_off, in_len, stream)


# ---- partial decode: the first target[i] bytes of every block (lz4flex_decompress_batch_partial) ------------------------------------
def decompress_batch_partial(in_buf, in_off, in_len, out_buf, out_off, target, ctx=None):
    """lz4flex_decompress_batch_partial over host buffers: the first min(size, target[i]) bytes of block in_buf[in_off[i] : + in_len[i]]
    into out_buf[out_off[i] : + target[i]]; nothing is written behind target[i] bytes of a sink.  Returns (out_len[u32], status[i32]):
    there is no OutputTooSmall and no detail."""
    return _host_call("lz4flex_decompress_batch_partial", ctx, in_buf, in_off, in_len, (out_buf, out_off, target))


def _partial_device(name, src, in_off, in_len, target, stream, after_n=(), tail=(), **companions):
    """The device recipe of the partial entries: the output is packed by an exclusive prefix sum of `target` (ONE host synchronisation:
    the total, to allocate exactly that), then one
        name(NULL, src, in_off, in_len, n, *after_n, out, out_off, target, out_len, status, *tail, mem_kind, stream)
    Returns (out, out_off, out_len, status)."""
    import torch
    dev, n, d_off, d_len, sp = _device_args(src, in_off, in_len, stream, **companions)
    if int(target.numel()) != n:
        raise ValueError("in_off and target differ in length")
    want = target.to(device=dev, dtype=torch.int64) & 0xFFFFFFFF
    out_off = torch.cumsum(want, 0) - want
    total = int(want.sum()) if n else 0                  # the one synchronisation
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    out_len = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    if n:
        d_target = torch.where(want >= 0x80000000, want - 0x100000000, want).to(torch.int32).contiguous()     # (the bit pattern of a u32)
        _device_call(name, [src, d_off, d_len], n, [*after_n, out, out_off, d_target, out_len, status, *tail], False, sp)
    return out[:total], out_off, out_len, status


def decompress_blocks_partial_device(src, in_off, in_len, target, stream=None):
    """Raw blocks in device memory, the first target[i] bytes of each: src is a uint8 torch tensor on the GPU, in_off / in_len / target
    integer tensors.  The output is packed by an exclusive prefix sum of `target` (ONE host synchronisation: the total, to allocate
    exactly that), then one lz4flex_decompress_batch_partial (MEM_DEVICE, asynchronous on `stream`, default the current one).  Returns
    (out, out_off, out_len, status) as device tensors: block i's bytes are out[out_off[i] : out_off[i] + out_len[i]], out_len[i] =
    min(size, target[i]); a block that fails in front of its target gets its status and out_len 0."""
    return _partial_device("lz4flex_decompress_batch_partial", src, in_off, in_len, target, stream)


# ---- per-block dictionaries (lz4flex_*_batch_ex) --------------------------------------------------------------------------------
def compress_batch_with_dict(in_buf, in_off, in_len, dict_buf, dict_off, dict_len, out_buf, out_off, out_cap, flags=None, ctx=None):
    """lz4flex_compress_batch_ex over host buffers: block i = in_buf[in_off[i] : + in_len[i]] compressed against the dictionary
    dict_buf[dict_off[i] : + dict_len[i]] (dict_len[i] == 0: none) into out_buf[out_off[i] : + out_cap[i]] -- block::compress_into_with_dict
    as a batch.  compress_mode exact gives the reference's bytes; fast (the default) the throughput encoder's, which use the dictionary's
    last 32 KiB; high gives fast's unless set_compress_high_dict(True), then a deep search of the block and of the dictionary's last
    32 KiB (the same holds for the shared-dictionary and the dictionary-set forms below).  Returns (out_len[u32], status[i32])."""
    ext, _keep = _host_dict_ext(L.CompressExt, dict_buf, dict_off, dict_len)
    return _host_call("lz4flex_compress_batch_ex", ctx, in_buf, in_off, in_len, (out_buf, out_off, out_cap), before_n=[_u32(flags)],
                      tail=[C.byref(ext)])


def decompress_batch_with_dict(in_buf, in_off, in_len, dict_buf, dict_off, dict_len, out_buf, out_off, out_cap, ctx=None):
    """lz4flex_decompress_batch_ex with per-block dictionaries over host buffers (block::decompress_into_with_dict as a batch):
    returns (out_len[u32], status[i32], detail[n,2] u64)."""
    ext, _keep = _host_dict_ext(L.DecompressExt, dict_buf, dict_off, dict_len)     # (no out_pos, no chains)
    return _host_call("lz4flex_decompress_batch_ex", ctx, in_buf, in_off, in_len, (out_buf, out_off, out_cap), tail=[C.byref(ext)],
                      detail=True)


def compress_blocks_with_dict_device(src, in_off, in_len, dicts, dict_off, dict_len, stream=None):
    """Blocks and dictionaries in device memory: src and dicts are uint8 torch tensors on the GPU, block i is src[in_off[i] : + in_len[i]]
    and its dictionary dicts[dict_off[i] : + dict_len[i]] (0: none).  One lz4flex_compress_batch_ex (MEM_DEVICE, asynchronous on `stream`,
    default the current one) into output slots of get_maximum_output_size(in_len[i]) bytes.  Returns (out, out_off, out_len, status) as
    device tensors: block i's bytes are out[out_off[i] : out_off[i] + out_len[i]]."""
    import torch
    n = int(in_off.numel())
    if int(dict_off.numel()) != n or int(dict_len.numel()) != n:
        raise ValueError("in_off, in_len, dict_off and dict_len differ in length")
    k_off = dict_off.to(device=src.device, dtype=torch.int64).contiguous()
    k_len = dict_len.to(device=src.device, dtype=torch.int32).contiguous()
    # (dict_base is not NULL, which would mean "no dictionaries": without dictionary bytes every dict_len is 0 and the address is not read)
    ext = L.CompressExt((dicts if dicts.numel() else k_len).data_ptr(), k_off.data_ptr(), k_len.data_ptr())
    return _compress_slots_device("lz4flex_compress_batch_ex", src, in_off, in_len, stream, before_n=[None], tail=[C.byref(ext)], dicts=dicts)


# ---- one dictionary for the batch (lz4flex_*_batch_shared_dict) ----------------------------------------------------------------
def compress_batch_with_shared_dict(in_buf, in_off, in_len, dictionary, out_buf, out_off, out_cap, ctx=None):
    """lz4flex_compress_batch_shared_dict over host buffers: every block in_buf[in_off[i] : + in_len[i]] is compressed against the ONE
    `dictionary` (bytes-like or a uint8 array) into out_buf[out_off[i] : + out_cap[i]] -- the bytes of compress_batch_with_dict with
    that dictionary for every block, with the work that depends on the dictionary alone done once per call.  Returns (out_len[u32],
    status[i32])."""
    d = _host_u8(dictionary)
    return _host_call("lz4flex_compress_batch_shared_dict", ctx, in_buf, in_off, in_len, (out_buf, out_off, out_cap), tail=[d, int(d.size)])


def compress_blocks_with_shared_dict_device(src, in_off, in_len, dictionary, stream=None):
    """Blocks and ONE dictionary in device memory: src and dictionary are uint8 torch tensors on the GPU, block i is
    src[in_off[i] : + in_len[i]].  One lz4flex_compress_batch_shared_dict (MEM_DEVICE, asynchronous on `stream`, default the current
    one) into output slots of get_maximum_output_size(in_len[i]) bytes.  Returns (out, out_off, out_len, status) as device tensors:
    block i's bytes are out[out_off[i] : out_off[i] + out_len[i]]."""
    return _compress_slots_device("lz4flex_compress_batch_shared_dict", src, in_off, in_len, stream,
                                  tail=[dictionary, int(dictionary.numel())], dictionary=dictionary)


def decompress_batch_with_shared_dict(in_buf, in_off, in_len, dictionary, out_buf, out_off, out_cap, ctx=None):
    """lz4flex_decompress_batch_shared_dict over host buffers: every block in_buf[in_off[i] : + in_len[i]] is decoded against the ONE
    `dictionary` (bytes-like or a uint8 array) into out_buf[out_off[i] : + out_cap[i]] -- the results of decompress_batch_with_dict with
    that dictionary for every block.  Returns (out_len[u32], status[i32], detail[n,2] u64)."""
    d = _host_u8(dictionary)
    return _host_call("lz4flex_decompress_batch_shared_dict", ctx, in_buf, in_off, in_len, (out_buf, out_off, out_cap),
                      tail=[d, int(d.size)], detail=True)


def decompress_blocks_with_shared_dict_device(src, in_off, in_len, dictionary, stream=None):
    """Raw blocks and their ONE dictionary in device memory, sizes unknown: the counterpart of decompress_blocks_device and the inverse
    of compress_blocks_with_shared_dict_device.  The size pass with the dictionary's length as every block's history, an exclusive prefix
    sum for the output offsets, ONE host synchronisation (the total, to allocate exactly that), one
    lz4flex_decompress_batch_shared_dict with out_cap = the sizes.  Returns (out, out_off, out_len, status) as device tensors: block i's
    bytes are out[out_off[i] : out_off[i] + out_len[i]]; a block that fails gets its status and an empty slot."""
    import torch
    dlen = int(dictionary.numel())
    hist = torch.full((int(in_off.numel()),), dlen, dtype=torch.int64, device=src.device).to(torch.int32)     # (the bit pattern of a u32)
    return _size_then_decode_device("lz4flex_decompress_batch_shared_dict", src, in_off, in_len, stream, history=hist,
                                    tail=[dictionary, dlen], dictionary=dictionary)


def decompress_batch_partial_with_shared_dict(in_buf, in_off, in_len, dictionary, out_buf, out_off, target, ctx=None):
    """lz4flex_decompress_batch_partial_shared_dict over host buffers: decompress_batch_partial for blocks that were compressed against
    the ONE `dictionary` (bytes-like or a uint8 array) -- the first min(size, target[i]) bytes of every block into out_buf[out_off[i] : +
    target[i]].  Returns (out_len[u32], status[i32])."""
    d = _host_u8(dictionary)
    return _host_call("lz4flex_decompress_batch_partial_shared_dict", ctx, in_buf, in_off, in_len, (out_buf, out_off, target),
                      tail=[d, int(d.size)])


def decompress_blocks_partial_with_shared_dict_device(src, in_off, in_len, target, dictionary, stream=None):
    """decompress_blocks_partial_device for blocks that were compressed against the ONE `dictionary` (a uint8 torch tensor on the GPU of
    src): one lz4flex_decompress_batch_partial_shared_dict into the same packed layout -- out_off is the exclusive prefix sum of
    `target`.  Returns (out, out_off, out_len, status) as device tensors."""
    return _partial_device("lz4flex_decompress_batch_partial_shared_dict", src, in_off, in_len, target, stream,
                           tail=[dictionary, int(dictionary.numel())], dictionary=dictionary)


# ---- dictionary sets: K prepared dictionaries, one id per block (lz4flex_dict_set_*, lz4flex_*_batch_dict_set) -------------
class DictSet:
    """lz4flex_dict_set: `dictionaries` (a sequence of bytes-like objects or uint8 arrays; an empty one means "no dictionary" for its
    id) copied to the device and digested once, reused by every compress_batch_with_dict_set / decompress_batch_with_dict_set call
    that names it.  A context manager; close() (or the end of the object) frees the device memory -- order it behind the work that
    uses the set.  len() is K."""

    def __init__(self, dictionaries, ctx=None):
        self._lib = L.load()
        self._h = C.c_void_p()
        parts = [_host_u8(d) for d in dictionaries]
        self.lengths = np.array([p.size for p in parts], dtype=np.uint32)
        offs = np.zeros(len(parts), dtype=np.uint64)
        if len(parts):
            offs[1:] = np.cumsum(self.lengths[:-1], dtype=np.uint64)
        flat = np.concatenate(parts) if len(parts) and int(self.lengths.sum()) else np.zeros(1, dtype=np.uint8)
        _check(self._lib.lz4flex_dict_set_create(ctx, _arg(flat), _arg(offs), _arg(self.lengths), len(parts), L.MEM_HOST, C.byref(self._h)),
               "lz4flex_dict_set_create")

    @property
    def handle(self):
        if not self._h:
            raise ValueError("the dictionary set is closed")
        return self._h

    def __len__(self):
        return int(self._lib.lz4flex_dict_set_count(self.handle))

    def close(self):
        h, self._h = self._h, C.c_void_p()
        if h:
            self._lib.lz4flex_dict_set_free(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def compress_batch_with_dict_set(in_buf, in_off, in_len, dict_id, dict_set, out_buf, out_off, out_cap, ctx=None):
    """lz4flex_compress_batch_dict_set over host buffers: block in_buf[in_off[i] : + in_len[i]] is compressed against dictionary
    dict_id[i] of `dict_set` (NO_DICT: none) into out_buf[out_off[i] : + out_cap[i]] -- the bytes of compress_batch_with_dict with that
    dictionary per block; only the batch and the ids travel to the device.  Returns (out_len[u32], status[i32])."""
    return _host_call("lz4flex_compress_batch_dict_set", ctx, in_buf, in_off, in_len, (out_buf, out_off, out_cap),
                      middle=[_host_ids(dict_id, len(in_off))], tail=[dict_set])


def decompress_batch_with_dict_set(in_buf, in_off, in_len, dict_id, dict_set, out_buf, out_off, out_cap, ctx=None):
    """lz4flex_decompress_batch_dict_set over host buffers: the mirror of compress_batch_with_dict_set -- the results of
    decompress_batch_with_dict with dictionary dict_id[i] per block.  Returns (out_len[u32], status[i32], detail[n,2] u64)."""
    return _host_call("lz4flex_decompress_batch_dict_set", ctx, in_buf, in_off, in_len, (out_buf, out_off, out_cap),
                      middle=[_host_ids(dict_id, len(in_off))], tail=[dict_set], detail=True)


def decompress_batch_partial_with_dict_set(in_buf, in_off, in_len, dict_id, dict_set, out_buf, out_off, target, ctx=None):
    """lz4flex_decompress_batch_partial_dict_set over host buffers: decompress_batch_partial with dictionary dict_id[i] of `dict_set`
    (NO_DICT: none) for block i.  Returns (out_len[u32], status[i32]); an id the set does not have gives that block E_INVALID_ARG."""
    return _host_call("lz4flex_decompress_batch_partial_dict_set", ctx, in_buf, in_off, in_len, (out_buf, out_off, target),
                      middle=[_host_ids(dict_id, len(in_off))], tail=[dict_set])


def _device_ids(dict_id, n, dev):
    """dict_id as n int64 on dev, and as the int32 bit pattern of n u32"""
    import torch
    if int(dict_id.numel()) != n:
        raise ValueError("in_off and dict_id differ in length")
    ids = dict_id.to(device=dev, dtype=torch.int64) & 0xFFFFFFFF
    return ids, torch.where(ids >= 0x80000000, ids - 0x100000000, ids).to(torch.int32).contiguous()


def compress_blocks_with_dict_set_device(src, in_off, in_len, dict_id, dict_set, stream=None):
    """Blocks in device memory against a DictSet: src is a uint8 torch tensor on the set's GPU, block i is src[in_off[i] : + in_len[i]],
    its dictionary dict_id[i] (NO_DICT: none).  One lz4flex_compress_batch_dict_set (MEM_DEVICE, asynchronous on `stream`, default the
    current one) into output slots of get_maximum_output_size(in_len[i]) bytes.  Returns (out, out_off, out_len, status) as device
    tensors: block i's bytes are out[out_off[i] : out_off[i] + out_len[i]]."""
    _, ids = _device_ids(dict_id, int(in_off.numel()), src.device)
    return _compress_slots_device("lz4flex_compress_batch_dict_set", src, in_off, in_len, stream, after_n=[ids], tail=[dict_set])


def decompress_blocks_with_dict_set_device(src, in_off, in_len, dict_id, dict_set, stream=None):
    """Raw blocks in device memory against a DictSet, sizes unknown: the inverse of compress_blocks_with_dict_set_device.  The size pass
    with each block's dictionary length as its history, an exclusive prefix sum for the output offsets, ONE host synchronisation (the
    total, to allocate exactly that), one lz4flex_decompress_batch_dict_set with out_cap = the sizes.  Returns (out, out_off, out_len,
    status) as device tensors; a block that fails gets its status and an empty slot (an id the set does not have: INVALID_ARG)."""
    import torch
    n, dev, hist = int(in_off.numel()), src.device, None
    ids64, ids = _device_ids(dict_id, n, dev)
    if n:
        # (an id without a dictionary -- NO_DICT, or one the set does not have: the decoder refuses that block -- has no history)
        lens = torch.cat([torch.from_numpy(dict_set.lengths.astype(np.int64)), torch.zeros(1, dtype=torch.int64)]).to(dev)
        k = len(dict_set)
        hist = lens[torch.where(ids64 < k, ids64, torch.full_like(ids64, k))].to(torch.int32)     # (the bit pattern of a u32)
    # (a refused id is the decoder's to report)
    return _size_then_decode_device("lz4flex_decompress_batch_dict_set", src, in_off, in_len, stream, history=hist, after_n=[ids],
                                    tail=[dict_set], decoder_wins=L.E_INVALID_ARG)


def decompress_blocks_partial_with_dict_set_device(src, in_off, in_len, target, dict_id, dict_set, stream=None):
    """decompress_blocks_partial_device against a DictSet: src is a uint8 torch tensor on the set's GPU, block i's dictionary is
    dict_id[i] (NO_DICT: none).  One lz4flex_decompress_batch_partial_dict_set into the same packed layout -- out_off is the exclusive
    prefix sum of `target`.  Returns (out, out_off, out_len, status) as device tensors (an id the set does not have: E_INVALID_ARG)."""
    _, ids = _device_ids(dict_id, int(in_off.numel()), src.device)
    return _partial_device("lz4flex_decompress_batch_partial_dict_set", src, in_off, in_len, target, stream, after_n=[ids], tail=[dict_set])


# ---- packed batches: one output buffer, the offsets computed on the device (lz4flex_*_batch_packed) ------------------------
def decompress_batch_packed(in_buf, in_off, in_len, out_buf, size_mode="prepended", sizes=None, align=1, total_cap=None, big_blocks=False,
                            ctx=None):
    """lz4flex_decompress_batch_packed over host buffers: block i = in_buf[in_off[i] : + in_len[i]] is decoded into out_buf, slot behind
    slot.  size_mode "prepended": the blocks carry block::compress_prepend_size's LE u32 (block::decompress_size_prepended as a batch);
    "given": sizes[i] is block i's capacity (block::decompress); "scan": raw blocks, measured on the device.  total_cap (default: all of
    out_buf) bounds what is written; a block whose slot ends behind it gets OutputTooSmall.  Returns (out_off[u64, n + 1], out_cap[u32],
    out_len[u32], status[i32], detail[n, 2] u64): block i's bytes are out_buf[out_off[i] : out_off[i] + out_len[i]], out_off[n] is the
    capacity the batch needs."""
    n = len(in_off)
    out_off, out_cap = np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    cap = int(out_buf.size) if total_cap is None else int(total_cap)
    return (out_off, out_cap) + _host_call("lz4flex_decompress_batch_packed", ctx, in_buf, in_off, in_len,
                                           middle=[SIZE_MODES[size_mode], _u32(sizes), out_buf, cap, int(align), out_off, out_cap], tail=[None],
                                           detail=True, mem_kind=L.MEM_HOST | (L.MEM_BIG_BLOCKS if big_blocks else 0))


def compress_batch_packed(in_buf, in_off, in_len, out_buf, prepend_size=True, align=1, total_cap=None, ctx=None):
    """lz4flex_compress_batch_packed over host buffers: the blocks in_buf[in_off[i] : + in_len[i]] compressed back to back into out_buf
    (prepend_size: each behind its LE u32 length, block::compress_prepend_size).  Returns (out_off[u64, n + 1], out_len[u32],
    status[i32]): block i's bytes are out_buf[out_off[i] : out_off[i] + out_len[i]], out_off[n] is the capacity the stream needs."""
    n, prefix, in_len = len(in_off), 1 if prepend_size else 0, _np(in_len, np.uint32)
    out_off = np.zeros(n + 1, dtype=np.uint64)
    cap = int(out_buf.size) if total_cap is None else int(total_cap)
    slots = int(L.load().lz4flex_compress_packed_scratch_bound(int(in_len.sum(dtype=np.uint64)), n, prefix))
    return (out_off,) + _host_call("lz4flex_compress_batch_packed", ctx, in_buf, in_off, in_len,
                                   middle=[prefix, None, slots, out_buf, cap, int(align), out_off], tail=[None])


def _packed_device_args(src, in_off, in_len, capacity, stream):
    """what the two packed device forms share: the prologue, and the tensors they return -- out (of max(capacity, 1) bytes), out_off
    (n + 1), out_len, status"""
    import torch
    dev, n, d_off, d_len, sp = _device_args(src, in_off, in_len, stream)
    return dev, n, d_off, d_len, sp, (torch.empty(max(capacity, 1), dtype=torch.uint8, device=dev),
                                      torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                                      torch.zeros(n, dtype=torch.int32, device=dev))


def decompress_blocks_packed_device(src, in_off, in_len, capacity, size_mode="prepended", sizes=None, align=1, big_blocks=False, stream=None,
                                    ctx=None):
    """Blocks in device memory, decoded into ONE buffer of `capacity` bytes whose layout is computed on the device: src is a uint8 torch
    tensor on the GPU, block i is src[in_off[i] : in_off[i] + in_len[i]] (size_mode as for decompress_batch_packed; "given": sizes is an
    integer tensor).  One lz4flex_decompress_batch_packed (MEM_DEVICE, asynchronous on `stream`, default the current one): no host
    synchronisation, nothing copied to the host.  Returns (out, out_off, out_len, status) as device tensors: out has `capacity` bytes,
    out_off n + 1 entries (the last one: the capacity the batch needs), block i's bytes are out[out_off[i] : out_off[i] + out_len[i]]; a
    block whose slot ends behind `capacity` has status E_OUTPUT_TOO_SMALL and nothing of it is written."""
    import torch
    capacity = int(capacity)
    dev, n, d_off, d_len, sp, (out, out_off, out_len, status) = _packed_device_args(src, in_off, in_len, capacity, stream)
    if n:
        out_cap = torch.empty(n, dtype=torch.int32, device=dev)
        d_sizes = None if sizes is None else sizes.to(device=dev, dtype=torch.int64).to(torch.int32).contiguous()
        work = torch.empty(int(L.load().lz4flex_packed_work_size(n)), dtype=torch.uint8, device=dev)
        _device_call("lz4flex_decompress_batch_packed", [src, d_off, d_len], n,
                     [SIZE_MODES[size_mode], d_sizes, out, capacity, int(align), out_off, out_cap, out_len, status, None, work],
                     big_blocks, sp, ctx)
    return out[:capacity], out_off, out_len, status


def compress_blocks_packed_device(src, in_off, in_len, capacity, prepend_size=True, align=1, big_blocks=False, scratch_cap=None, stream=None,
                                  ctx=None):
    """Blocks in device memory, compressed back to back into ONE buffer of `capacity` bytes: src is a uint8 torch tensor on the GPU, block
    i is src[in_off[i] : in_off[i] + in_len[i]]; prepend_size: every block behind its LE u32 length (block::compress_prepend_size).  One
    lz4flex_compress_batch_packed (MEM_DEVICE, asynchronous on `stream`, default the current one): no host synchronisation.  The scratch
    slots are sized for blocks that together have no more bytes than src (scratch_cap: another capacity; blocks whose slots end behind
    it get E_OUTPUT_TOO_SMALL).  big_blocks: the batch may hold blocks of more than 64 KiB (compress_mode exact needs to know).  Returns
    (out, out_off, out_len, status) as device tensors: out has `capacity` bytes, out_off n + 1 entries (the last one: the capacity the
    stream needs), block i's bytes are out[out_off[i] : out_off[i] + out_len[i]] -- what decompress_blocks_packed_device reads."""
    import torch
    capacity, prefix = int(capacity), 1 if prepend_size else 0
    dev, n, d_off, d_len, sp, (out, out_off, out_len, status) = _packed_device_args(src, in_off, in_len, capacity, stream)
    if n:
        lib = L.load()
        if scratch_cap is None:
            scratch_cap = int(lib.lz4flex_compress_packed_scratch_bound(int(src.numel()), n, prefix))
        scratch = torch.empty(max(int(scratch_cap), 1), dtype=torch.uint8, device=dev)
        work = torch.empty(int(lib.lz4flex_packed_work_size(n)), dtype=torch.uint8, device=dev)
        _device_call("lz4flex_compress_batch_packed", [src, d_off, d_len], n,
                     [prefix, scratch, int(scratch_cap), out, capacity, int(align), out_off, out_len, status, work], big_blocks, sp, ctx)
    return out[:capacity], out_off, out_len, status


# ---- a dictionary from the data (lz4flex_dict_train) ---------------------------------------------------------------------------
def train_dictionary_batch(in_buf, in_off, in_len, dict_size=32768, segment=512, ctx=None):
    """lz4flex_dict_train over host buffers: a dictionary of at most dict_size (<= 65 536) bytes cut from the samples in_buf[in_off[i] :
    + in_len[i]], in segments of at most `segment` bytes (64 ... 2 048) -- the ones whose 8-byte windows are the most frequent in the
    whole batch, the best at the tail.  The bytes are a function of the samples, dict_size and segment alone.  Returns bytes: what
    DictSet([...]), the *_with_shared_dict calls and *_with_dict take."""
    out = np.zeros(max(int(dict_size), 1), dtype=np.uint8)
    length, status = _host_call("lz4flex_dict_train", ctx, in_buf, in_off, in_len, middle=[out, int(dict_size), int(segment)], tail=[None],
                                per_call=True)
    if status[0]:
        raise ValueError("train_dictionary: the samples have 2^32 positions or more (status %d)" % status[0])
    return out[:int(length[0])].tobytes()


def train_dictionary(samples, dict_size=32768, segment=512, ctx=None):
    """train_dictionary_batch of a list of bytes-likes (or uint8 arrays)."""
    parts = [_host_u8(s) for s in samples]
    lens = np.array([p.size for p in parts], dtype=np.uint32)
    offs = np.zeros(len(parts), dtype=np.uint64)
    if len(parts):
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    flat = np.concatenate(parts) if len(parts) and int(lens.sum(dtype=np.uint64)) else np.zeros(1, dtype=np.uint8)
    return train_dictionary_batch(flat, offs, lens, dict_size, segment, ctx)


def train_dictionary_device(src, in_off, in_len, dict_size=32768, segment=512, stream=None):
    """Samples in device memory: src is a uint8 torch tensor on the GPU, sample i is src[in_off[i] : + in_len[i]].  One lz4flex_dict_train
    (MEM_DEVICE, asynchronous on `stream`, default the current one; the workspace of lz4flex_dict_train_work_size(n) bytes is allocated
    here): no host synchronisation, nothing copied to the host.  Returns (dictionary, dict_len) as device tensors: dictionary has
    dict_size bytes of which the first dict_len[0] are the dictionary (dictionary[:int(dict_len)] is what the *_shared_dict_device calls
    take)."""
    import torch
    dict_size = int(dict_size)
    dev, n, d_off, d_len, sp = _device_args(src, in_off, in_len, stream)
    out = torch.zeros(max(dict_size, 1), dtype=torch.uint8, device=dev)
    res = torch.zeros(2, dtype=torch.int32, device=dev)          # dict_len, status
    work = torch.empty(int(L.load().lz4flex_dict_train_work_size(n)), dtype=torch.uint8, device=dev)
    _device_call("lz4flex_dict_train", [src, d_off, d_len], n, [out, dict_size, int(segment), res[0:1], res[1:2], work], False, sp)
    return out[:dict_size], res[0:1]


# ---- typed batches: byte- and bit-shuffle filters around the codec (lz4flex_filter_batch, lz4flex_*_batch_typed) -----------------
FILTERS = {"none": L.FILTER_NONE, "shuffle": L.FILTER_SHUFFLE, "bitshuffle": L.FILTER_BITSHUFFLE}


def _filter_args(filter, elem_size, delta=False):
    """(filter, elem_size) as the C ABI takes them: "none" | "shuffle" | "bitshuffle" or 0 / 1 / 2, an element of 1, 2, 4 or 8 bytes;
    delta (a bool) ORs LZ4FLEX_FILTER_DELTA into the filter"""
    if not isinstance(delta, bool):
        raise ValueError("delta must be a bool, not %r" % (delta,))
    if isinstance(filter, str):
        if filter not in FILTERS:
            raise ValueError("filter must be one of %s or 0 / 1 / 2, not %r" % (", ".join(map(repr, FILTERS)), filter))
        filter = FILTERS[filter]
    elif isinstance(filter, bool) or not isinstance(filter, (int, np.integer)) or int(filter) not in FILTERS.values():
        raise ValueError("filter must be one of %s or 0 / 1 / 2, not %r" % (", ".join(map(repr, FILTERS)), filter))
    if isinstance(elem_size, bool) or not isinstance(elem_size, (int, np.integer)) or int(elem_size) not in (1, 2, 4, 8):
        raise ValueError("elem_size must be 1, 2, 4 or 8, not %r" % (elem_size,))
    return int(filter) | (L.FILTER_DELTA if delta else 0), int(elem_size)


def _same_length(in_off, **others):
    for name, a in others.items():
        if len(a) != len(in_off):
            raise ValueError("in_off and %s differ in length" % name)


def filter_batch(in_buf, in_off, in_len, out_buf, out_off, filter, elem_size, inverse=False, ctx=None, delta=False):
    """lz4flex_filter_batch over host buffers: block i = in_buf[in_off[i] : + in_len[i]] goes through `filter` ("none" | "shuffle" |
    "bitshuffle" or 0 / 1 / 2) for elements of elem_size bytes -- inverse: through its inverse -- into out_buf[out_off[i] : + in_len[i]]
    (a uint8 array).  delta=True puts the difference stage (LZ4FLEX_FILTER_DELTA: element minus its neighbour, restarting every 1 024
    elements) in front of the filter.  The transforms are defined in include/lz4flex_amd.h.  Returns None."""
    f, e = _filter_args(filter, elem_size, delta)
    _same_length(in_off, in_len=in_len, out_off=out_off)
    _host_call("lz4flex_filter_batch", ctx, in_buf, in_off, in_len, middle=[out_buf, _np(out_off, np.uint64)], tail=[f, e, 1 if inverse else 0],
               results=False)


def compress_batch_typed(in_buf, in_off, in_len, out_buf, out_off, out_cap, filter, elem_size, ctx=None, delta=False):
    """lz4flex_compress_batch_typed over host buffers: every block is filtered (filter_batch), then compressed as compress_batch does
    it -- out_buf, out_len and status are compress_batch's for the filtered bytes.  delta: as in filter_batch.  Returns (out_len[u32],
    status[i32])."""
    f, e = _filter_args(filter, elem_size, delta)
    _same_length(in_off, in_len=in_len, out_off=out_off, out_cap=out_cap)
    return _host_call("lz4flex_compress_batch_typed", ctx, in_buf, in_off, in_len, (out_buf, out_off, out_cap), tail=[f, e, None, None])


def decompress_batch_typed(in_buf, in_off, in_len, out_buf, out_off, out_cap, filter, elem_size, ctx=None, delta=False):
    """lz4flex_decompress_batch_typed over host buffers: every block is decoded as decompress_batch does it and, where its status is 0,
    the inverse filter of its out_len[i] bytes goes to out_buf[out_off[i] : + out_len[i]]; a block that fails writes nothing.  Returns
    (out_len[u32], status[i32], detail[n,2] u64): decompress_batch's.  delta: what the blocks were compressed with."""
    f, e = _filter_args(filter, elem_size, delta)
    _same_length(in_off, in_len=in_len, out_off=out_off, out_cap=out_cap)
    return _host_call("lz4flex_decompress_batch_typed", ctx, in_buf, in_off, in_len, (out_buf, out_off, out_cap), detail=True,
                      tail=[f, e, None, None])


def filter_blocks_device(src, in_off, in_len, filter, elem_size, inverse=False, stream=None, delta=False):
    """Blocks in device memory through a filter (inverse: its inverse): src is a uint8 torch tensor on the GPU, block i is src[in_off[i] :
    in_off[i] + in_len[i]].  One lz4flex_filter_batch (MEM_DEVICE, asynchronous on `stream`, default the current one): no host
    synchronisation.  Returns (out, out_off): out has src's size, out_off = in_off -- block i's bytes are out[out_off[i] : out_off[i] +
    in_len[i]], what lies between the blocks is not written.  delta: as in filter_batch."""
    import torch
    f, e = _filter_args(filter, elem_size, delta)
    dev, n, d_off, d_len, sp = _device_args(src, in_off, in_len, stream)
    out = torch.empty_like(src)
    if n:
        _device_call("lz4flex_filter_batch", [src, d_off, d_len], n, [out, d_off, f, e, 1 if inverse else 0], False, sp)
    return out, d_off


def compress_blocks_typed_device(src, in_off, in_len, filter, elem_size, stream=None, delta=False):
    """Blocks of numeric data in device memory, filtered and compressed: src is a uint8 torch tensor on the GPU, block i is src[in_off[i] :
    in_off[i] + in_len[i]], elements of elem_size bytes.  One lz4flex_compress_batch_typed (MEM_DEVICE, asynchronous on `stream`, default
    the current one) into slots of get_maximum_output_size(in_len[i]) bytes; the tmp slots are a second tensor of src's size.  Returns
    (out, out_off, out_len, status) as device tensors: block i's bytes are out[out_off[i] : out_off[i] + out_len[i]].  delta: as in
    filter_batch."""
    import torch
    f, e = _filter_args(filter, elem_size, delta)
    tmp_off = _device_args(src, in_off, in_len, stream)[2]
    tmp = torch.empty_like(src)
    return _compress_slots_device("lz4flex_compress_batch_typed", src, in_off, in_len, stream, tail=[f, e, tmp, tmp_off])


def decompress_blocks_typed_device(src, in_off, in_len, out_cap, filter, elem_size, stream=None, delta=False):
    """What compress_blocks_typed_device wrote, back to the numeric data: src is a uint8 torch tensor on the GPU, block i is src[in_off[i] :
    in_off[i] + in_len[i]] and decodes to at most out_cap[i] bytes (an integer tensor).  The output is packed by an exclusive prefix sum of
    out_cap (ONE host synchronisation: the total, to allocate the output and the tmp slots), then one lz4flex_decompress_batch_typed
    (MEM_DEVICE, asynchronous on `stream`, default the current one).  Returns (out, out_off, out_len, status) as device tensors: block i's
    bytes are out[out_off[i] : out_off[i] + out_len[i]]; a block that fails gets its status and nothing of it is written.  delta: what
    the blocks were compressed with."""
    import torch
    f, e = _filter_args(filter, elem_size, delta)
    dev, n, d_off, d_len, sp = _device_args(src, in_off, in_len, stream)
    if int(out_cap.numel()) != n:
        raise ValueError("in_off and out_cap differ in length")
    cap = out_cap.to(device=dev, dtype=torch.int64) & 0xFFFFFFFF
    out_off = torch.cumsum(cap, 0) - cap
    total, longest = (int(v) for v in torch.stack([cap.sum(), d_len.max()]).cpu()) if n else (0, 0)      # the one synchronisation
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    out_len = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    if n:
        tmp = torch.empty_like(out)
        d_cap = torch.where(cap >= 0x80000000, cap - 0x100000000, cap).to(torch.int32).contiguous()      # (the bit pattern of a u32)
        _device_call("lz4flex_decompress_batch_typed", [src, d_off, d_len], n, [out, out_off, d_cap, out_len, status, None, f, e, tmp, out_off],
                     longest > 131072, sp)
    return out[:total], out_off, out_len, status


# ---- fit batches: compress into a fixed capacity (lz4flex_fit_batch, lz4flex_compress_batch_fit) --------------------------------------
def fit_batch(blk_buf, blk_off, blk_len, src_buf, src_off, src_len, out_buf, out_off, out_cap, ctx=None):
    """lz4flex_fit_batch over host buffers: the finished block blk_buf[blk_off[i] : + blk_len[i]], which decodes to src_buf[src_off[i] : +
    src_len[i]], cut to at most out_cap[i] bytes at out_buf[out_off[i]:] (a uint8 array) -- the block itself when it fits, else the
    valid block inside the capacity that decodes to the longest prefix of the source (the rule: include/lz4flex_amd.h).  Returns
    (out_len[u32], in_used[u32], status[i32]): block i's bytes are out_buf[out_off[i] : out_off[i] + out_len[i]] and decode to the first
    in_used[i] source bytes; an error of the block in front of the cut is its status, out_cap[i] == 0 gives E_OUTPUT_TOO_SMALL."""
    _same_length(blk_off, blk_len=blk_len, src_off=src_off, src_len=src_len, out_off=out_off, out_cap=out_cap)
    return _host_call("lz4flex_fit_batch", ctx, blk_buf, blk_off, blk_len, (out_buf, out_off, out_cap),
                      before_n=[_host_u8(src_buf), _np(src_off, np.uint64), _np(src_len, np.uint32)], in_used=True)


def compress_batch_fit(in_buf, in_off, in_len, out_buf, out_off, out_cap, ctx=None):
    """lz4flex_compress_batch_fit over host buffers: every block in_buf[in_off[i] : + in_len[i]] is compressed as compress_batch does it
    (compress_mode as set) and cut to out_cap[i] bytes as fit_batch does it.  Returns (out_len[u32], in_used[u32], status[i32]); out_cap[i]
    >= get_maximum_output_size(in_len[i]) gives compress_batch's bytes and in_used[i] = in_len[i].  The encoder encodes all of every
    block whatever its capacity."""
    _same_length(in_off, in_len=in_len, out_off=out_off, out_cap=out_cap)
    return _host_call("lz4flex_compress_batch_fit", ctx, in_buf, in_off, in_len, (out_buf, out_off, out_cap), middle=[None, 0], tail=[None],
                      in_used=True)


def compress_fit(data, cap):
    """`data` compressed into at most `cap` bytes (LZ4_compress_destSize; a batch of one): (block, used) -- block decodes to data[:used]."""
    cap = int(cap)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    src = _host_u8(data)
    out_len, used, status = compress_batch_fit(src if src.size else np.zeros(1, dtype=np.uint8), [0], [src.size], out, [0], [cap])
    if status[0] == L.E_OUTPUT_TOO_SMALL:
        raise CompressOutputTooSmall("no LZ4 block fits %d bytes" % cap)
    if status[0]:
        raise DeviceError("lz4flex error %d: %s" % (status[0], L.last_error()))
    return out[:int(out_len[0])].tobytes(), int(used[0])


def _fit_slots_device(dev, n, out_cap):
    """the output of the two fit device forms: slots of out_cap[i] bytes back to back (ONE host synchronisation: the total, to allocate
    exactly that).  Returns (out, out_off, out_cap as the int32 bit pattern of u32, out_len, in_used, status)."""
    import torch
    if int(out_cap.numel()) != n:
        raise ValueError("in_off and out_cap differ in length")
    cap = out_cap.to(device=dev, dtype=torch.int64) & 0xFFFFFFFF
    out_off = torch.cumsum(cap, 0) - cap
    total = int(cap.sum()) if n else 0
    d_cap = torch.where(cap >= 0x80000000, cap - 0x100000000, cap).to(torch.int32).contiguous()
    return (torch.empty(max(total, 1), dtype=torch.uint8, device=dev)[:total], out_off, d_cap, torch.zeros(n, dtype=torch.int32, device=dev),
            torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))


def fit_blocks_device(blocks, blk_off, blk_len, src, src_off, src_len, out_cap, stream=None):
    """Finished blocks and their sources in device memory, cut to out_cap[i] bytes each: blocks and src are uint8 torch tensors on one
    GPU, block i is blocks[blk_off[i] : + blk_len[i]] and decodes to src[src_off[i] : + src_len[i]].  The output is packed by an exclusive
    prefix sum of out_cap (ONE host synchronisation: the total), then one lz4flex_fit_batch (MEM_DEVICE, asynchronous on `stream`,
    default the current one).  Returns (out, out_off, out_len, in_used, status) as device tensors: block i's bytes are out[out_off[i] :
    out_off[i] + out_len[i]] and decode to the first in_used[i] bytes of its source."""
    import torch
    dev, n, b_off, b_len, sp = _device_args(blocks, blk_off, blk_len, stream, source=src)
    if int(src_off.numel()) != n or int(src_len.numel()) != n:
        raise ValueError("blk_off, src_off and src_len differ in length")
    s_off = src_off.to(device=dev, dtype=torch.int64).contiguous()
    s_len = src_len.to(device=dev, dtype=torch.int32).contiguous()
    out, out_off, d_cap, out_len, used, status = _fit_slots_device(dev, n, out_cap)
    if n:
        _device_call("lz4flex_fit_batch", [blocks, b_off, b_len, src, s_off, s_len], n, [out, out_off, d_cap, out_len, used, status], False, sp)
    return out, out_off, out_len, used, status


def compress_blocks_fit_device(src, in_off, in_len, out_cap, stream=None, scratch_cap=None):
    """Blocks in device memory, compressed into out_cap[i] bytes each: src is a uint8 torch tensor on the GPU, block i is src[in_off[i] :
    in_off[i] + in_len[i]].  The output is packed by an exclusive prefix sum of out_cap (ONE host synchronisation: the total and the
    longest block), then one lz4flex_compress_batch_fit (MEM_DEVICE, asynchronous on `stream`, default the current one); the scratch slots
    and the workspace are allocated here, by torch's allocator on the CURRENT stream, and released on return as in the other device forms:
    a `stream` other than the current one has to be ordered with it by the caller.  scratch_cap: another capacity for the scratch slots
    (default: what always suffices); blocks whose slot ends behind it get E_OUTPUT_TOO_SMALL.  Returns (out, out_off, out_len, in_used,
    status) as device tensors: block i's bytes are out[out_off[i] : out_off[i] + out_len[i]] and decode to src[in_off[i] : in_off[i] +
    in_used[i]]."""
    import torch
    dev, n, d_off, d_len, sp = _device_args(src, in_off, in_len, stream, wide_len=True)
    out, out_off, d_cap, out_len, used, status = _fit_slots_device(dev, n, out_cap)
    if n:
        lib = L.load()
        total_in, longest = (int(v) for v in torch.stack([d_len.sum(), d_len.max()]).cpu())
        scratch_cap = int(lib.lz4flex_compress_packed_scratch_bound(total_in, n, 0)) if scratch_cap is None else int(scratch_cap)
        scratch = torch.empty(max(scratch_cap, 1), dtype=torch.uint8, device=dev)
        work = torch.empty(int(lib.lz4flex_compress_fit_work_size(n)), dtype=torch.uint8, device=dev)
        _device_call("lz4flex_compress_batch_fit", [src, d_off, d_len.to(torch.int32)], n,
                     [scratch, scratch_cap, out, out_off, d_cap, out_len, used, status, work], longest > 65536, sp)
    return out, out_off, out_len, used, status


# ---- paged streams: every stream cut into pages of page_size bytes (lz4flex_compress_paged) -----------------------------------------------
class PagedStreams:
    """What compress_paged / compress_paged_device return and decompress_paged / decompress_paged_device take: the page file `pages` (page
    e is pages[e * page_size : e * page_size + page_len[e]], a self-contained LZ4 block that decodes to the stream's bytes from page_src[e]
    on), the table page_len / page_src, stream i's entries [page_off[i], page_off[i] + n_pages[i]), and per stream in_done (the bytes its
    pages hold) and status (0, or the code the stream ended with: its pages so far stay valid).  numpy arrays from the host form, device
    tensors from the device form."""
    __slots__ = ("page_size", "pages", "page_off", "page_len", "page_src", "n_pages", "in_done", "status")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])


def paged_pages_bound(in_len, page_size):
    """lz4flex_paged_pages_bound: the pages that always suffice for a stream of in_len bytes"""
    return int(L.load().lz4flex_paged_pages_bound(int(in_len), int(page_size)))


def paged_rounds_bound(max_in_len, page_size, window_min=0, window_max=0):
    """lz4flex_paged_rounds_bound: the max_rounds that always suffices for streams of at most max_in_len bytes"""
    return int(L.load().lz4flex_paged_rounds_bound(int(max_in_len), int(page_size), int(window_min), int(window_max)))


def _paged_windows(page_size, window_min, window_max):
    """the windows with the header's defaults resolved (the checks are the library's)"""
    window_min = int(window_min) or 4 * int(page_size)
    return window_min, int(window_max) or max(window_min, 65536)


def compress_paged(streams, page_size, page_cap=None, window_min=0, window_max=0, max_rounds=None, ctx=None):
    """lz4flex_compress_paged over host bytes: every stream (bytes-like) cut into pages of page_size bytes, each page a self-contained LZ4
    block that holds as much of its stream as fits (the rule: include/lz4flex_amd.h; compress_mode as set).  page_cap: the pages stream i
    may take (default: paged_pages_bound, which always suffices); max_rounds default: paged_rounds_bound of the longest stream.  Returns a
    PagedStreams of numpy arrays; a stream that ran out of pages or rounds has status E_OUTPUT_TOO_SMALL and valid pages so far."""
    page_size = int(page_size)
    parts = [_host_u8(s) for s in streams]
    n = len(parts)
    in_len = np.array([p.size for p in parts], dtype=np.uint32)
    in_off = np.zeros(n, dtype=np.uint64)
    if n:
        in_off[1:] = np.cumsum(in_len[:-1], dtype=np.uint64)
    src = np.concatenate(parts + [np.zeros(1, dtype=np.uint8)])
    cap = [paged_pages_bound(v, page_size) for v in in_len] if page_cap is None else [int(v) for v in page_cap]
    if len(cap) != n:
        raise ValueError("streams and page_cap differ in length")
    page_off = np.zeros(n + 1, dtype=np.uint64)
    page_off[1:] = np.cumsum(np.array(cap, dtype=np.uint64))
    entries = int(page_off[n])
    if max_rounds is None:
        max_rounds = paged_rounds_bound(int(in_len.max()) if n else 0, page_size, window_min, window_max)
    res = PagedStreams(page_size=page_size, pages=np.zeros(max(entries * page_size, 1), dtype=np.uint8)[:entries * page_size], page_off=page_off,
                       page_len=np.zeros(entries, dtype=np.uint32), page_src=np.zeros(entries, dtype=np.uint32),
                       n_pages=np.zeros(n, dtype=np.uint32), in_done=np.zeros(n, dtype=np.uint32), status=np.zeros(n, dtype=np.int32))
    keep = [np.zeros(1, dtype=np.uint32) if a.size == 0 else a for a in (res.pages, res.page_len, res.page_src)]     # (an empty table still needs an address)
    args = [src, in_off, in_len, n, page_size, int(window_min), int(window_max), int(max_rounds), keep[0], page_off, keep[1], keep[2],
            res.n_pages, res.in_done, res.status, None, 0, None]
    _check(L.load().lz4flex_compress_paged(ctx, *map(_arg, args), L.MEM_HOST, None), "lz4flex_compress_paged")
    return res


def decompress_paged(paged, ctx=None):
    """The streams of a PagedStreams (host form) back as a list of bytes -- stream i's first in_done[i] bytes -- with ONE decompress_batch
    over the page table: page e of stream i decodes to [page_src[e], page_src[e + 1]) of it (the last page: up to in_done[i])."""
    P = int(paged.page_size)
    n = len(paged.n_pages)
    base = np.zeros(n + 1, dtype=np.uint64)
    base[1:] = np.cumsum(paged.in_done.astype(np.uint64))
    in_off, in_len, out_off, out_cap = [], [], [], []
    for i in range(n):
        first, k = int(paged.page_off[i]), int(paged.n_pages[i])
        starts = [int(v) for v in paged.page_src[first:first + k]] + [int(paged.in_done[i])]
        for j in range(k):
            in_off.append((first + j) * P)
            in_len.append(int(paged.page_len[first + j]))
            out_off.append(int(base[i]) + starts[j])
            out_cap.append(starts[j + 1] - starts[j])
    out = np.zeros(max(int(base[n]), 1), dtype=np.uint8)
    if in_off:
        out_len, status, _ = decompress_batch(paged.pages, in_off, in_len, out, out_off, out_cap, ctx=ctx)
        bad = np.nonzero((status != 0) | (out_len != np.array(out_cap, dtype=np.uint32)))[0]
        if bad.size:
            raise DecompressError("page entry %d does not decode to its slice (status %d)" % (in_off[int(bad[0])] // P, int(status[bad[0]])))
    return [out[int(base[i]):int(base[i + 1])].tobytes() for i in range(n)]


def compress_paged_device(src, in_off, in_len, page_size, page_cap=None, window_min=0, window_max=0, max_rounds=None, stream=None,
                          scratch_cap=None):
    """Streams in device memory cut into pages: src is a uint8 torch tensor on the GPU, stream i is src[in_off[i] : in_off[i] + in_len[i]].
    page_cap (an integer tensor; default: lz4flex_paged_pages_bound of every length, computed on the device) gives the page table by an
    exclusive prefix sum; ONE host synchronisation for the sizes (the entries, the longest stream, the scratch the windows need), then one
    lz4flex_compress_paged (MEM_DEVICE, asynchronous on `stream`, default the current one: max_rounds rounds are enqueued, default the
    rounds bound of the longest stream).  Scratch and workspace are allocated here, by torch's allocator on the CURRENT stream, as in the
    other device forms.  Returns a PagedStreams of device tensors (page_len / page_src / n_pages / in_done: the int32 bit patterns of u32)."""
    import torch
    page_size = int(page_size)
    dev, n, d_off, d_len, sp = _device_args(src, in_off, in_len, stream, wide_len=True)
    lib = L.load()
    window_min_r, window_max_r = _paged_windows(page_size, window_min, window_max)
    if page_cap is None:
        # lz4flex_paged_pages_bound(len) = ceil(len / lfit) for every length at once: lfit is the longest stream that takes one page
        y = page_size - 17
        lfit = 15 + y - y // 256 - (1 if y % 256 == 255 else 0)
        if paged_pages_bound(lfit, page_size) != 1 or paged_pages_bound(lfit + 1, page_size) != 2:
            raise ValueError("page_size %d: not a page size of lz4flex_compress_paged" % page_size)
        cap = (d_len + (lfit - 1)) // lfit
    else:
        if int(page_cap.numel()) != n:
            raise ValueError("in_off and page_cap differ in length")
        cap = page_cap.to(device=dev, dtype=torch.int64)
    page_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n:
        page_off[1:] = torch.cumsum(cap, 0)
        entries, longest, offered = (int(v) for v in torch.stack([page_off[n], d_len.max(), torch.clamp(d_len, max=window_max_r).sum()]).cpu())
    else:
        entries = longest = offered = 0
    i32 = lambda m: torch.zeros(m, dtype=torch.int32, device=dev)     # noqa: E731
    res = PagedStreams(page_size=page_size, pages=torch.empty(max(entries * page_size, 1), dtype=torch.uint8, device=dev)[:entries * page_size],
                       page_off=page_off, page_len=i32(entries), page_src=i32(entries), n_pages=i32(n), in_done=i32(n), status=i32(n))
    if n:
        if max_rounds is None:
            max_rounds = paged_rounds_bound(longest, page_size, window_min, window_max)
        scratch_cap = int(lib.lz4flex_compress_packed_scratch_bound(offered, n, 0)) if scratch_cap is None else int(scratch_cap)
        scratch = torch.empty(max(scratch_cap, 1), dtype=torch.uint8, device=dev)
        work = torch.empty(int(lib.lz4flex_compress_paged_work_size(n)), dtype=torch.uint8, device=dev)
        keep = [i32(1) if t.numel() == 0 else t for t in (res.pages, res.page_len, res.page_src)]
        _device_call("lz4flex_compress_paged", [src, d_off, d_len.to(torch.int32)], n,
                     [page_size, int(window_min), int(window_max), int(max_rounds), keep[0], page_off, keep[1], keep[2], res.n_pages, res.in_done,
                      res.status, scratch, scratch_cap, work], min(longest, window_max_r) > 65536, sp)
    return res


def decompress_paged_device(paged, stream=None):
    """The streams of a PagedStreams (device form) back in device memory, with ONE lz4flex_decompress_batch over the page table (the
    table is turned into the batch's arrays by torch, with one host synchronisation for the number of committed pages and the total).
    Returns (out, out_off, out_len, status): stream i's bytes are out[out_off[i] : out_off[i] + out_len[i]], out_len = in_done; status
    is per stream, 0 or the largest code one of its pages failed with (a page that decodes to another length than its slice counts as
    E_OUTPUT_TOO_SMALL)."""
    import torch
    P = int(paged.page_size)
    dev = paged.pages.device
    n = int(paged.n_pages.numel())
    done = paged.in_done.to(torch.int64) & 0xFFFFFFFF
    out_off = torch.cumsum(done, 0) - done
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    entries = int(paged.page_len.numel())
    if n == 0 or entries == 0:
        return torch.empty(0, dtype=torch.uint8, device=dev), out_off, done, status
    first = paged.page_off[:n].to(torch.int64)
    e = torch.arange(entries, dtype=torch.int64, device=dev)
    owner = torch.clamp(torch.searchsorted(paged.page_off.to(torch.int64).contiguous(), e, right=True) - 1, 0, n - 1)
    k = e - first[owner]
    pages_of = (paged.n_pages.to(torch.int64) & 0xFFFFFFFF)[owner]
    live = torch.nonzero(k < pages_of).flatten()                    # (a synchronisation: the committed pages)
    start = (paged.page_src.to(torch.int64) & 0xFFFFFFFF)
    nxt = torch.cat([start[1:], start[:1]])
    end = torch.where(k + 1 < pages_of, nxt, done[owner])
    b_off = (live * P).contiguous()
    b_len = paged.page_len[live].contiguous()
    b_out = (out_off[owner] + start)[live].contiguous()
    b_cap = (end - start)[live].to(torch.int32).contiguous()
    total = int(done.sum())
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    m = int(live.numel())
    if m:
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        b_got, b_st = torch.zeros(m, dtype=torch.int32, device=dev), torch.zeros(m, dtype=torch.int32, device=dev)
        _device_call("lz4flex_decompress_batch", [paged.pages, b_off, b_len], m, [out, b_out, b_cap, b_got, b_st, None], P > 131072, C.c_void_p(stream))
        b_st = torch.where((b_st == 0) & (b_got != b_cap), torch.full_like(b_st, L.E_OUTPUT_TOO_SMALL), b_st)
        status.scatter_reduce_(0, owner[live], b_st, "amax", include_self=True)
    return out[:total], out_off, done, status


def paged_range_pages_bound(length, page_size):
    """lz4flex_paged_range_pages_bound: the pages a range of `length` bytes can touch in tables compress_paged wrote"""
    return int(L.load().lz4flex_paged_range_pages_bound(int(length), int(page_size)))


def _paged_tables(paged):
    """the five tables of a PagedStreams as lz4flex_paged_read_ranges takes them (an empty one still gets an address)"""
    keep = [paged.pages, paged.page_off, paged.page_len, paged.page_src, paged.n_pages, paged.in_done]
    if isinstance(paged.pages, np.ndarray):
        keep = [_host_u8(keep[0]), _np(keep[1], np.uint64)] + [_np(a, np.uint32) for a in keep[2:]]
        return [np.zeros(1, dtype=a.dtype) if a.size == 0 else a for a in keep]
    return [a.new_zeros(1) if a.numel() == 0 else a.contiguous() for a in keep]


def read_paged_ranges(paged, sid, off, length, ctx=None):
    """lz4flex_paged_read_ranges over a PagedStreams of numpy arrays (MEM_HOST): range r is bytes [off[r], off[r] + length[r]) of stream
    sid[r], clipped at the stream's in_done; length 0xFFFFFFFF with off 0 reads a whole stream.  Returns (list of bytes, status): the
    bytes of a range with status != 0 are b"" (status: the rule's codes, include/lz4flex_amd.h)."""
    sid, off, length = _np(sid, np.uint32), _np(off, np.uint32), _np(length, np.uint32)
    m = len(sid)
    if len(off) != m or len(length) != m:
        raise ValueError("sid, off and length differ in length")
    pages, page_off, page_len, page_src, n_pages, in_done = _paged_tables(paged)
    n = len(paged.n_pages)
    out_len, status = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.int32)
    if m == 0:
        return [], status
    done = np.array([int(paged.in_done[i]) if i < n else 0 for i in sid], dtype=np.int64)
    room = np.clip(np.minimum(length.astype(np.int64), done - off.astype(np.int64)), 0, None)
    out_off = np.zeros(m, dtype=np.uint64)
    out_off[1:] = np.cumsum(room[:-1])
    out = np.zeros(max(int(room.sum()), 1), dtype=np.uint8)
    args = [pages, int(paged.page_size), page_off, page_len, page_src, n_pages, in_done, n, sid, off, length, m, out, out_off, out_len, status,
            0, None, 0, None]
    _check(L.load().lz4flex_paged_read_ranges(ctx, *map(_arg, args), L.MEM_HOST, None), "lz4flex_paged_read_ranges")
    return [out[int(o):int(o) + int(k)].tobytes() for o, k in zip(out_off, out_len)], status


def read_paged_ranges_device(paged, sid, off, length, out=None, out_off=None, max_items=None, scratch_cap=None, stream=None):
    """lz4flex_paged_read_ranges over a PagedStreams of device tensors (MEM_DEVICE, asynchronous on `stream`, default the current one):
    sid / off / length are integer tensors (the low 32 bits count) or anything torch.as_tensor takes.  Nothing is read back from the
    device unless a default needs it: out / out_off default to regions of min(length[r], in_done - off[r]) bytes back to back, computed
    on the device (ONE synchronisation, for their sum; length 0xFFFFFFFF with off 0 reads whole streams); max_items defaults to the sum
    of paged_range_pages_bound(length[r]) when `length` is host-visible, else to the number of table entries plus m -- and never to
    more than that, which suffices for ranges that do not overlap; scratch_cap defaults to the default window_max of 65536 bytes per
    range, 1 GiB at most (real needs are about one page's decoded size per head).  A range the capacities do not serve reports
    E_OUTPUT_TOO_SMALL: pass larger ones.  Scratch and work come from torch's allocator on the CURRENT stream, as in the other device
    forms.  Returns (out, out_off, out_len, status): range r's bytes are out[out_off[r] : out_off[r] + out_len[r]]; out_len / status
    as int32 tensors (the bit patterns of u32 / the rule's codes)."""
    import torch
    dev = paged.pages.device
    P = int(paged.page_size)
    host_len = None if hasattr(length, "data_ptr") and length.device.type != "cpu" else [int(v) & 0xFFFFFFFF for v in np.asarray(length).reshape(-1)]

    def u32(a):
        # wrap-around intended: the library reads the bit pattern
        a = torch.as_tensor(np.asarray(a, dtype=np.int64) if not hasattr(a, "data_ptr") else a)
        return ((a.to(device=dev, dtype=torch.int64) + 0x80000000) % 0x100000000 - 0x80000000).to(torch.int32).contiguous()

    d_sid, d_off, d_len = u32(sid), u32(off), u32(length)
    m = int(d_sid.numel())
    if int(d_off.numel()) != m or int(d_len.numel()) != m:
        raise ValueError("sid, off and length differ in length")
    n = int(paged.n_pages.numel())
    out_len, status = torch.zeros(m, dtype=torch.int32, device=dev), torch.zeros(m, dtype=torch.int32, device=dev)
    if out is None or out_off is None:
        if out is not None or out_off is not None:
            raise ValueError("out and out_off come together")
        # every region as long as the range can get: min(length, in_done - off) needs the tables, which are on the device -- computed there
        done = torch.cat([paged.in_done.to(torch.int64) & 0xFFFFFFFF, torch.zeros(1, dtype=torch.int64, device=dev)])
        idx = torch.clamp(d_sid.to(torch.int64) & 0xFFFFFFFF, max=n)
        room = torch.clamp(torch.minimum(d_len.to(torch.int64) & 0xFFFFFFFF, done[idx] - (d_off.to(torch.int64) & 0xFFFFFFFF)), min=0)
        out_off = torch.cumsum(room, 0) - room
        out = torch.empty(max(int(room.sum()) if m else 0, 1), dtype=torch.uint8, device=dev)     # (a synchronisation: the output's size)
    else:
        if out.device != dev or out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError("out must be a contiguous uint8 tensor on the GPU of the pages")
        out_off = out_off.to(device=dev, dtype=torch.int64).contiguous()
        if int(out_off.numel()) != m:
            raise ValueError("sid and out_off differ in length")
    if m == 0:
        return out, out_off, out_len, status
    lib = L.load()
    if max_items is None:
        entries = int(paged.page_len.numel())
        max_items = entries + m
        if host_len is not None:
            max_items = min(max_items, sum(paged_range_pages_bound(v, P) for v in host_len))
    max_items = min(int(max_items), 0xFFFFFFFF)
    scratch_cap = min(m * 65536, 1 << 30) if scratch_cap is None else int(scratch_cap)
    scratch = torch.empty(max(scratch_cap, 1), dtype=torch.uint8, device=dev)
    work = torch.empty(int(lib.lz4flex_paged_read_work_size(m, max_items)), dtype=torch.uint8, device=dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    pages, page_off, page_len, page_src, n_pages, in_done = _paged_tables(paged)
    _device_call("lz4flex_paged_read_ranges", [pages, P, page_off.to(torch.int64), page_len, page_src, n_pages, in_done], n,
                 [d_sid, d_off, d_len, m, out, out_off, out_len, status, max_items, scratch, scratch_cap, work], P > 131072, C.c_void_p(stream))
    return out, out_off, out_len, status


# ---- paged streams, append: new bytes for any subset of the streams (lz4flex_paged_append) ------------------------------------------------
NO_STAGE = 0xFFFFFFFFFFFFFFFF     # stage_off[i] of a stream without a stage slot


def paged_append_stage_bound(sum_add_len, n, page_size, window_min=0, window_max=0):
    """lz4flex_paged_append_stage_bound: a stage_cap that always suffices for n streams that get sum_add_len new bytes in all.  The
    windows are resolved here as lz4flex_paged_append resolves them for page_size (0: the defaults), so the bound and a call with the
    same arguments agree; 0 for windows the entry refuses."""
    return int(L.load().lz4flex_paged_append_stage_bound(int(sum_add_len), int(n), _paged_windows(page_size, window_min, window_max)[1]))


def reserve_paged(paged, page_cap):
    """The same streams in a table with room for page_cap[i] entries per stream (compress_paged sizes its table exactly by default, which
    leaves no room to append): page_off becomes the exclusive sums of page_cap from 0, every committed page and its entry move to their
    new places.  Host form (numpy arrays) or device form (torch tensors; one synchronisation for the sizes), as `paged` is.  A page_cap[i]
    below n_pages[i] is a ValueError.  Plain indexing, not a kernel.  Returns a new PagedStreams; `paged` is not changed."""
    P = int(paged.page_size)
    n = len(paged.n_pages)
    if isinstance(paged.pages, np.ndarray):
        cap = _np(page_cap, np.int64)
        k = paged.n_pages.astype(np.int64)
        if len(cap) != n:
            raise ValueError("the streams and page_cap differ in length")
        if (cap < k).any():
            raise ValueError("page_cap is below n_pages")
        new_off = np.zeros(n + 1, dtype=np.uint64)
        new_off[1:] = np.cumsum(cap)
        entries, total = int(new_off[n]), int(k.sum())
        owner = np.repeat(np.arange(n), k)
        j = np.arange(total) - np.repeat(np.cumsum(k) - k, k)
        old, new = paged.page_off[:n].astype(np.int64)[owner] + j, new_off[:n].astype(np.int64)[owner] + j
        pages = np.zeros(max(entries * P, 1), dtype=np.uint8)[:entries * P]
        page_len, page_src = np.zeros(entries, dtype=np.uint32), np.zeros(entries, dtype=np.uint32)
        if total:
            pages.reshape(entries, P)[new] = _host_u8(paged.pages)[:(int(old.max()) + 1) * P].reshape(-1, P)[old]
            page_len[new], page_src[new] = paged.page_len[old], paged.page_src[old]
        return PagedStreams(page_size=P, pages=pages, page_off=new_off, page_len=page_len, page_src=page_src, n_pages=paged.n_pages.copy(),
                            in_done=paged.in_done.copy(), status=paged.status.copy())
    import torch
    dev = paged.pages.device
    cap = torch.as_tensor(page_cap).to(device=dev, dtype=torch.int64)
    k = paged.n_pages.to(torch.int64) & 0xFFFFFFFF
    if int(cap.numel()) != n:
        raise ValueError("the streams and page_cap differ in length")
    new_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n:
        new_off[1:] = torch.cumsum(cap, 0)
    short, entries, total = (int(v) for v in torch.stack([(cap < k).sum(), new_off[n], k.sum()]).cpu()) if n else (0, 0, 0)
    if short:
        raise ValueError("page_cap is below n_pages")
    pages = torch.zeros(max(entries * P, 1), dtype=torch.uint8, device=dev)[:entries * P]
    page_len, page_src = (torch.zeros(entries, dtype=torch.int32, device=dev) for _ in range(2))
    if total:
        owner = torch.repeat_interleave(torch.arange(n, device=dev), k, output_size=total)
        j = torch.arange(total, device=dev) - (torch.cumsum(k, 0) - k)[owner]
        old, new = paged.page_off[:n].to(torch.int64)[owner] + j, new_off[:n][owner] + j
        pages.view(entries, P)[new] = paged.pages[:(int(paged.pages.numel()) // P) * P].view(-1, P)[old]
        page_len[new], page_src[new] = paged.page_len[old], paged.page_src[old]
    return PagedStreams(page_size=P, pages=pages, page_off=new_off, page_len=page_len, page_src=page_src, n_pages=paged.n_pages.clone(),
                        in_done=paged.in_done.clone(), status=paged.status.clone())


def append_paged(paged, adds, window_min=0, window_max=0, max_rounds=None, ctx=None):
    """lz4flex_paged_append over a PagedStreams of numpy arrays (MEM_HOST): adds[i] (bytes-like; empty: none) goes behind stream i, whose
    last page is reopened and filled up before new pages are begun (the rule: include/lz4flex_amd.h).  The table needs room behind
    n_pages[i] for the pages to come: reserve_paged.  max_rounds default: what always suffices.  `paged` is updated in place -- pages,
    table, n_pages, in_done, status -- and returned; a stream that ran out of pages or rounds has status E_OUTPUT_TOO_SMALL and a valid
    prefix of in_done[i] bytes (which may be fewer than before the call: the rest of the reopened page is lost to the host form)."""
    P = int(paged.page_size)
    n = len(paged.n_pages)
    parts = [_host_u8(a) for a in adds]
    if len(parts) != n:
        raise ValueError("the streams and adds differ in length")
    add_len = np.array([p.size for p in parts], dtype=np.uint32)
    add_off = np.zeros(n, dtype=np.uint64)
    if n:
        add_off[1:] = np.cumsum(add_len[:-1], dtype=np.uint64)
    src = np.concatenate(parts + [np.zeros(1, dtype=np.uint8)])
    pages, page_off, page_len, page_src, n_pages, in_done = _paged_tables(paged)
    for name, a, b in (("pages", pages, paged.pages), ("page_len", page_len, paged.page_len), ("page_src", page_src, paged.page_src),
                       ("n_pages", n_pages, paged.n_pages), ("in_done", in_done, paged.in_done)):
        if b.size and (a is not b or not b.flags.c_contiguous or (name == "pages" and b.dtype != np.uint8)):
            raise ValueError("%s must be a contiguous array of the table's type: the call updates it in place" % name)
    if max_rounds is None:
        wmax = _paged_windows(P, window_min, window_max)[1]
        max_rounds = paged_rounds_bound(min(wmax + (int(add_len.max()) if n else 0), 0xFFFFFFFF), P, window_min, window_max)
    status = np.zeros(n, dtype=np.int32)
    stage_off, tail_src = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    args = [src, add_off, add_len, n, P, int(window_min), int(window_max), int(max_rounds), pages, page_off, page_len, page_src, n_pages, in_done,
            status, None, 0, stage_off, tail_src, None, 0, None]
    _check(L.load().lz4flex_paged_append(ctx, *map(_arg, args), L.MEM_HOST, None), "lz4flex_paged_append")
    paged.status = status
    return paged


def _device_u32(a, dev):
    """an integer tensor (or anything numpy converts) as the int32 bit pattern of u32 on `dev`: the low 32 bits count"""
    import torch
    a = torch.as_tensor(np.asarray(a, dtype=np.int64) if not hasattr(a, "data_ptr") else a)
    return ((a.to(device=dev, dtype=torch.int64) + 0x80000000) % 0x100000000 - 0x80000000).to(torch.int32).contiguous()


def append_paged_device(paged, src, add_off, add_len, window_min=0, window_max=0, max_rounds=None, stage_cap=None, scratch_cap=None, stream=None):
    """lz4flex_paged_append over a PagedStreams of device tensors (MEM_DEVICE, asynchronous on `stream`, default the current one): stream i
    gets the add_len[i] bytes src[add_off[i] : add_off[i] + add_len[i]] (src: a uint8 tensor on the pages' GPU; 0: none).  The table
    needs room behind n_pages[i]: reserve_paged.  Nothing is read back unless a default needs it, and then in ONE synchronisation: the
    defaults of max_rounds, stage_cap and scratch_cap are lz4flex_paged_rounds_bound, the stage slots and
    lz4flex_compress_packed_scratch_bound for the tails the tables name (T_i = in_done - page_src of the last entry, clamped to window_max)
    and the new bytes -- never more than lz4flex_paged_append_stage_bound and the header's scratch bound.  Stage, scratch and work come
    from torch's allocator on the CURRENT stream, as in the other device forms.  `paged` is updated in place.  Returns (paged, stage,
    stage_off, tail_src): after a nonzero status from the rounds the bytes of stream i that are not paged yet are
    stage[stage_off[i] + in_done[i] - tail_src[i] : ...]; stage_off as int64 (-1: no slot), tail_src as the int32 bit pattern of u32."""
    import torch
    P = int(paged.page_size)
    dev = paged.pages.device
    dev_, n, d_off, d_len64, sp = _device_args(src, add_off, add_len, stream, wide_len=True)
    if dev_ != dev:
        raise ValueError("src must be on the GPU of the pages")
    if int(paged.n_pages.numel()) != n:
        raise ValueError("the streams and add_off differ in length")
    for name in ("pages", "page_len", "page_src", "n_pages", "in_done"):
        if not getattr(paged, name).is_contiguous():
            raise ValueError("%s must be contiguous: the call updates it in place" % name)
    d_len = _device_u32(d_len64, dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    stage_off = torch.full((n,), -1, dtype=torch.int64, device=dev)
    tail_src = torch.zeros(n, dtype=torch.int32, device=dev)
    if n == 0:
        return paged, torch.empty(0, dtype=torch.uint8, device=dev), stage_off, tail_src
    lib = L.load()
    wmin, wmax = _paged_windows(P, window_min, window_max)
    longest = None
    if max_rounds is None or stage_cap is None or scratch_cap is None:
        A = d_len.to(torch.int64) & 0xFFFFFFFF
        k = paged.n_pages.to(torch.int64) & 0xFFFFFFFF
        first = paged.page_off[:n].to(torch.int64)
        entries = int(paged.page_src.numel())
        last = torch.clamp(first + k - 1, 0, max(entries - 1, 0))
        src_last = (paged.page_src.to(torch.int64) & 0xFFFFFFFF)[last] if entries else torch.zeros_like(k)
        T = torch.where(k > 0, torch.clamp((paged.in_done.to(torch.int64) & 0xFFFFFFFF) - src_last, 0, wmax), torch.zeros_like(k))
        V = torch.where(A > 0, T + A, torch.zeros_like(A))
        longest, slots, offered = (int(v) for v in torch.stack([V.max(), ((V + 63) // 64 * 64).sum(), torch.clamp(V, max=wmax).sum()]).cpu())
        if max_rounds is None:
            max_rounds = paged_rounds_bound(min(longest, 0xFFFFFFFF), P, window_min, window_max)
        if stage_cap is None:
            stage_cap = slots
        if scratch_cap is None:
            scratch_cap = int(lib.lz4flex_compress_packed_scratch_bound(offered, n, 0))
    stage_cap, scratch_cap = int(stage_cap), int(scratch_cap)
    stage = torch.empty(max(stage_cap, 1), dtype=torch.uint8, device=dev)
    scratch = torch.empty(max(scratch_cap, 1), dtype=torch.uint8, device=dev)
    work = torch.empty(int(lib.lz4flex_paged_append_work_size(n)), dtype=torch.uint8, device=dev)
    keep = [t.new_zeros(1) if t.numel() == 0 else t for t in (paged.pages, paged.page_len, paged.page_src)]
    big = wmax > 65536 if longest is None else min(longest, wmax) > 65536
    _device_call("lz4flex_paged_append", [src, d_off, d_len], n,
                 [P, int(window_min), int(window_max), int(max_rounds), keep[0], paged.page_off.to(torch.int64).contiguous(), keep[1], keep[2],
                  paged.n_pages, paged.in_done, status, stage, stage_cap, stage_off, tail_src, scratch, scratch_cap, work], big, sp)
    paged.status = status
    return paged, stage[:stage_cap], stage_off, tail_src


class CompressedTensor:
    """What compress_tensor returns and decompress_tensor takes: the compressed blocks back to back in `data` (a uint8 device tensor),
    block i at data[offsets[i] : offsets[i] + lengths[i]] (device tensors), and what the tensor was: shape, dtype, the block_bytes it was
    cut into, the filter (0 / 1 / 2) its blocks went through, and whether the delta stage ran in front of it."""
    __slots__ = ("data", "offsets", "lengths", "shape", "dtype", "block_bytes", "filter", "delta")

    def __init__(self, data, offsets, lengths, shape, dtype, block_bytes, filter, delta=False):
        self.data, self.offsets, self.lengths, self.shape, self.dtype = data, offsets, lengths, tuple(shape), dtype
        self.block_bytes, self.filter, self.delta = int(block_bytes), int(filter), bool(delta)

    @property
    def compressed_bytes(self):
        return int(self.data.numel())


def _tensor_blocks(total, block_bytes, dev):
    """a buffer of `total` bytes cut into blocks of block_bytes (the last one shorter): (in_off, in_len) as int64 device tensors"""
    import torch
    n = (total + block_bytes - 1) // block_bytes
    off = torch.arange(n, dtype=torch.int64, device=dev) * block_bytes
    return off, torch.clamp(total - off, max=block_bytes)


def compress_tensor(t, block_bytes=65536, filter="bitshuffle", delta=False):
    """A contiguous device tensor of a dtype of 1, 2, 4 or 8 bytes, compressed: its bytes are cut into blocks of block_bytes (a multiple of
    the element size), every block goes through `filter` for elements of t.element_size() bytes and the encoder (compress_mode as set).
    delta=True differences the elements as integers first (monotone integer columns: timestamps, sorted ids; no gain for floating point).
    Returns a CompressedTensor; decompress_tensor gives the tensor back bit for bit.  Raises ValueError for a dtype of another size, a
    tensor that is not contiguous or not on the GPU, a block_bytes the element size does not divide."""
    import torch
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or not t.is_contiguous():
        raise ValueError("compress_tensor takes a contiguous tensor on the GPU")
    f, e = _filter_args(filter, 1, delta)[0] & ~L.FILTER_DELTA, t.element_size()
    if e not in (1, 2, 4, 8):
        raise ValueError("compress_tensor takes dtypes of 1, 2, 4 or 8 bytes, not %s (%d bytes)" % (t.dtype, e))
    block_bytes = int(block_bytes)
    if block_bytes <= 0 or block_bytes % e or block_bytes > 0x7FFFFFFF:
        raise ValueError("block_bytes must be a positive multiple of the element size (%d) below 2 GiB, not %d" % (e, block_bytes))
    src = t.reshape(-1).view(torch.uint8)
    dev, total = t.device, int(src.numel())
    in_off, in_len = _tensor_blocks(total, block_bytes, dev)
    n = int(in_off.numel())
    if n == 0:
        empty = torch.empty(0, dtype=torch.int64, device=dev)
        return CompressedTensor(torch.empty(0, dtype=torch.uint8, device=dev), empty, empty.to(torch.int32), t.shape, t.dtype, block_bytes, f, delta)
    out, out_off, out_len, status = compress_blocks_typed_device(src, in_off, in_len, f, e, delta=delta)
    lens = out_len.to(torch.int64)
    offsets = torch.cumsum(lens, 0) - lens
    bad, size = (int(v) for v in torch.stack([(status != 0).sum(), lens.sum()]).cpu())
    if bad:
        raise CompressError("compress_tensor: %d of %d blocks failed" % (bad, n))
    data = torch.empty(max(size, 1), dtype=torch.uint8, device=dev)
    _check(L.load().lz4flex_copy_batch_device(_arg(out), _arg(out_off), _arg(out_len), _arg(data), _arg(offsets), n,
                                              C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "lz4flex_copy_batch_device")
    return CompressedTensor(data[:size], offsets, out_len, t.shape, t.dtype, block_bytes, f, delta)


def decompress_tensor(rec):
    """The tensor a CompressedTensor holds, on the GPU of its data, bit for bit."""
    import torch
    e = torch.empty(0, dtype=rec.dtype).element_size()
    count = 1
    for d in rec.shape:
        count *= int(d)
    total, dev = count * e, rec.data.device
    if total == 0:
        return torch.empty(rec.shape, dtype=rec.dtype, device=dev)
    _, caps = _tensor_blocks(total, rec.block_bytes, dev)
    if int(caps.numel()) != int(rec.offsets.numel()):
        raise ValueError("decompress_tensor: %d blocks for a tensor of %d" % (int(rec.offsets.numel()), int(caps.numel())))
    out, _, out_len, status = decompress_blocks_typed_device(rec.data, rec.offsets, rec.lengths, caps, rec.filter, e, delta=rec.delta)
    bad = int(((status != 0) | (out_len.to(torch.int64) != caps)).sum())
    if bad:
        raise DecompressError("decompress_tensor: %d of %d blocks failed" % (bad, int(caps.numel())))
    return out.view(rec.dtype).reshape(rec.shape)
