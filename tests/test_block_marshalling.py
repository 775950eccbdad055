"""CPU: what lz4_flex_amd.block's batched host forms hand to the C ABI, and what they hand back.

No GPU and no built library: _lib.load is replaced by a stand-in that takes every symbol's argument count and kinds from
_lib.SIGNATURES (ctypes converts each argument exactly as for the real library) and names the arguments as include/lz4flex_amd.h
declares them (PARAMS below).  A call is recorded by READING through its host pointers -- the descriptor arrays as n u64 / u32, the
blocks and dictionaries as the bytes the descriptors select, the ext structures field by field -- and answered by WRITING distinct
values through every output pointer.  A wrapper that swaps two arguments, converts to the wrong dtype or returns an array other than
the one it passed fails here, on any machine."""
import ctypes as C

import numpy as np
import pytest

from lz4_flex_amd import _lib as L
from lz4_flex_amd import block

_SPINE = "ctx in_base in_off in_len n out_base out_off out_cap out_len status"
PARAMS = {k: v.split() for k, v in {     # include/lz4flex_amd.h, in its order
    "lz4flex_compress_batch": "ctx in_base in_off in_len flags n out_base out_off out_cap out_len status mem_kind stream",
    "lz4flex_compress_batch_ex": "ctx in_base in_off in_len flags n out_base out_off out_cap out_len status ext mem_kind stream",
    "lz4flex_compress_batch_shared_dict": _SPINE + " dict dict_len mem_kind stream",
    "lz4flex_decompress_batch": _SPINE + " detail mem_kind stream",
    "lz4flex_decompress_batch_ex": _SPINE + " detail ext mem_kind stream",
    "lz4flex_decompress_batch_shared_dict": _SPINE + " detail dict dict_len mem_kind stream",
    "lz4flex_compress_batch_dict_set": "ctx in_base in_off in_len n dict_id out_base out_off out_cap out_len status set mem_kind stream",
    "lz4flex_decompress_batch_dict_set": "ctx in_base in_off in_len n dict_id out_base out_off out_cap out_len status detail set "
                                         "mem_kind stream",
    "lz4flex_decompressed_size_batch": "ctx in_base in_off in_len n history out_size status mem_kind stream",
    "lz4flex_decompress_batch_packed": "ctx in_base in_off in_len n size_mode sizes out_base total_cap align out_off out_cap out_len "
                                       "status detail work mem_kind stream",
    "lz4flex_compress_batch_packed": "ctx in_base in_off in_len n prepend_size scratch scratch_cap out_base total_cap align out_off "
                                     "out_len status work mem_kind stream",
}.items()}
OTHERS = ("lz4flex_dict_set_create", "lz4flex_dict_set_count", "lz4flex_dict_set_free", "lz4flex_compress_packed_scratch_bound")
HANDLE = 0x5E7D1C70
SCRATCH_BOUND = 0x123456789        # (more than 32 bits: scratch_cap is a u64)
MARK = 0xC3
LAST_ERROR = "the stand-in's last error"


# what the stand-in writes: distinct per array and per element, detail and the sizes beyond 32 bits
def w_out_len(n):
    return [1000 + i for i in range(n)]


def w_status(n):
    return [-(7 + i) for i in range(n)]


def w_detail(n):
    return [[(1 << 40) + 10 * i, (1 << 41) + 10 * i + 1] for i in range(n)]


def w_size(n):
    return [(1 << 42) + i for i in range(n)]


def w_packed_off(n):
    return [(1 << 33) + 16 * i for i in range(n + 1)]


def w_packed_cap(n):
    return [500 + i for i in range(n)]


def _read(ptr, ctype, count):
    return None if not ptr else list((ctype * count).from_address(ptr))


def _write(ptr, ctype, values):
    if ptr:
        (ctype * len(values)).from_address(ptr)[:] = values


def _bytes(base, off, length):
    if not length:
        return b""
    assert base, "a block of %d bytes behind a NULL base" % length
    return C.string_at(base + off, length)


def _select(base, off, length):
    return None if off is None or length is None else [_bytes(base, o, m) for o, m in zip(off, length)]


class StandIn:
    """lz4_flex_amd._lib.load()'s return value"""

    def __init__(self):
        self.calls, self.sets, self.freed, self.bounds, self.errors, self.rc = [], [], [], [], [], 0
        self._fns = {}
        for name in tuple(PARAMS) + OTHERS:
            res, args = L.SIGNATURES[name]
            if name in PARAMS:
                assert len(PARAMS[name]) == len(args), name
            self._fns[name] = self._bind(name, C.CFUNCTYPE(res, *args), len(args))

    def _bind(self, name, proto, count):
        handler = getattr(self, "_" + name, None) or (lambda *a: self._batched(name, *a))

        def guarded(*a):
            try:
                return handler(*a)
            except BaseException as e:      # (ctypes would swallow it: the fixture raises it after the test)
                self.errors.append(e)
                return -999
        fn = proto(guarded)

        def call(*a):
            if len(a) != count:             # (ctypes itself lets a cdecl function take more)
                raise TypeError("%s takes %d arguments (%d given)" % (name, count, len(a)))
            return fn(*a)
        return call

    def __getattr__(self, name):
        fns = self.__dict__.get("_fns", {})
        if name not in fns:
            raise AttributeError(name)
        return fns[name]

    def _batched(self, name, *args):
        a = dict(zip(PARAMS[name], args))
        n, packed = a["n"], name.endswith("_packed")
        r = dict(a, name=name)
        r["in_off"], r["in_len"] = _read(a["in_off"], C.c_uint64, n), _read(a["in_len"], C.c_uint32, n)
        r["blocks"] = _select(a["in_base"], r["in_off"], r["in_len"])
        for k in ("flags", "dict_id", "sizes", "history"):
            if k in a:
                r[k] = _read(a[k], C.c_uint32, n)
        if "dict" in a:
            r["dict"] = _bytes(a["dict"], 0, a["dict_len"]) if a["dict"] else None
        if "ext" in a:
            e = a["ext"].contents
            r["ext"] = {f: getattr(e, f) for f, _ in e._fields_}
            r["dicts"] = _select(e.dict_base, _read(e.dict_off, C.c_uint64, n), _read(e.dict_len, C.c_uint32, n))
        if packed:
            _write(a["out_off"], C.c_uint64, w_packed_off(n))
            if "out_cap" in a:
                _write(a["out_cap"], C.c_uint32, w_packed_cap(n))
            if a["out_base"] and a["total_cap"]:
                _write(a["out_base"], C.c_uint8, [MARK])
        elif "out_base" in a:
            r["out_off"], r["out_cap"] = _read(a["out_off"], C.c_uint64, n), _read(a["out_cap"], C.c_uint32, n)
            for o, c in zip(r["out_off"] or [], r["out_cap"] or []):
                if c:
                    _write(a["out_base"] + o, C.c_uint8, [MARK])
        _write(a.get("out_len"), C.c_uint32, w_out_len(n))
        _write(a.get("out_size"), C.c_uint64, w_size(n))
        _write(a["status"], C.c_int32, w_status(n))
        _write(a.get("detail"), C.c_uint64, [v for pair in w_detail(n) for v in pair])
        self.calls.append(r)
        return self.rc

    def _lz4flex_dict_set_create(self, ctx, dict_base, dict_off, dict_len, k, mem_kind, out):
        off, length = _read(dict_off, C.c_uint64, k), _read(dict_len, C.c_uint32, k)
        self.sets.append(dict(ctx=ctx, dict_base=dict_base, k=k, mem_kind=mem_kind, off=off, len=length,
                              dicts=_select(dict_base, off or [], length or []), flat=_bytes(dict_base, 0, sum(length or []))))
        if self.rc == 0:
            out[0] = HANDLE
        return self.rc

    def _lz4flex_dict_set_count(self, h):
        assert h == HANDLE
        return self.sets[-1]["k"]

    def _lz4flex_dict_set_free(self, h):
        self.freed.append(h)

    def _lz4flex_compress_packed_scratch_bound(self, total, n, prepend):
        self.bounds.append((total, n, prepend))
        return SCRATCH_BOUND


@pytest.fixture
def lib(monkeypatch):
    s = StandIn()
    monkeypatch.setattr(L, "load", lambda: s)
    monkeypatch.setattr(L, "last_error", lambda: LAST_ERROR)
    yield s
    if s.errors:
        raise s.errors[0]


# ---------------------------------------------------------------- the batch every test passes
IN_BYTES = b"###alpha#gamma-gamma##"
IN_OFF, IN_LEN = [3, 8, 9], [5, 0, 11]
BLOCKS = [b"alpha", b"", b"gamma-gamma"]
OUT_OFF, OUT_CAP = [1, 30, 31], [20, 0, 40]
DICT_BYTES = b"..first-dictionary.third"
DICT_OFF, DICT_LEN = [2, 0, 19], [16, 0, 5]
DICTS = [b"first-dictionary", b"", b"third"]
SHARED = b"one dictionary for all"
IDS = [2, block.NO_DICT, 0]
FLAGS = [0, 2, 3]
KINDS = ["ndarray", "list", "int64"]


def arr(values, dtype, kind, n=3):
    """the first n of `values` as the wrapper's documented dtype, as a list of ints, or as an array the wrapper has to convert"""
    values = values[:n]
    if kind == "list":
        return [int(v) for v in values]
    return np.array(values, dtype=np.int64 if kind == "int64" else dtype)


def u8(b, kind="ndarray"):
    return bytes(b) if kind == "list" else np.frombuffer(bytes(b), np.uint8).copy()


def the_set():
    return block.DictSet([u8(b"zero"), b"", b"two"])


SPINE = {      # form: (symbol, what stands between in_len and out_buf, detail?)
    "compress_batch": ("lz4flex_compress_batch", "", False),
    "decompress_batch": ("lz4flex_decompress_batch", "", True),
    "compress_batch_with_dict": ("lz4flex_compress_batch_ex", "dicts", False),
    "decompress_batch_with_dict": ("lz4flex_decompress_batch_ex", "dicts", True),
    "compress_batch_with_shared_dict": ("lz4flex_compress_batch_shared_dict", "shared", False),
    "decompress_batch_with_shared_dict": ("lz4flex_decompress_batch_shared_dict", "shared", True),
    "compress_batch_with_dict_set": ("lz4flex_compress_batch_dict_set", "set", False),
    "decompress_batch_with_dict_set": ("lz4flex_decompress_batch_dict_set", "set", True),
}
SYMBOL = dict({k: v[0] for k, v in SPINE.items()}, decompressed_size_batch="lz4flex_decompressed_size_batch",
              decompress_batch_packed="lz4flex_decompress_batch_packed", compress_batch_packed="lz4flex_compress_batch_packed")


def call_spine(form, kind="ndarray", n=3, in_buf=None, out_buf=None, dict_buf=None, shared=SHARED, ids=None, dict_set=None, **kw):
    """one call of a form on the out_off / out_cap spine: (what it returned, out_buf)"""
    middle = SPINE[form][1]
    if in_buf is None:
        in_buf = u8(IN_BYTES, "ndarray" if form == "decompress_batch" else kind)      # (decompress_batch takes an array only)
    out_buf = np.zeros(80, np.uint8) if out_buf is None else out_buf
    args = [in_buf, arr(IN_OFF, np.uint64, kind, n), arr(IN_LEN, np.uint32, kind, n)]
    if middle == "dicts":
        args += [u8(DICT_BYTES, kind) if dict_buf is None else dict_buf, arr(DICT_OFF, np.uint64, kind, n), arr(DICT_LEN, np.uint32, kind, n)]
    elif middle == "shared":
        args += [u8(shared, kind)]
    elif middle == "set":
        args += [arr(IDS, np.uint32, kind, n) if ids is None else ids, dict_set or the_set()]
    args += [out_buf, arr(OUT_OFF, np.uint64, kind, n), arr(OUT_CAP, np.uint32, kind, n)]
    return getattr(block, form)(*args, **kw), out_buf


def check_outputs(res, n, detail):
    """the returned arrays are the ones the C side wrote: dtype, shape, values"""
    assert len(res) == (3 if detail else 2)
    assert res[0].dtype == np.uint32 and res[0].shape == (n,) and res[0].tolist() == w_out_len(n)
    assert res[1].dtype == np.int32 and res[1].shape == (n,) and res[1].tolist() == w_status(n)
    if detail:
        assert res[2].dtype == np.uint64 and res[2].shape == (n, 2) and res[2].tolist() == w_detail(n)


def check_descriptors(r, n, names=("in_off", "in_len", "out_off", "out_cap")):
    want = dict(in_off=IN_OFF, in_len=IN_LEN, out_off=OUT_OFF, out_cap=OUT_CAP)
    for k in names:
        assert r[k] == want[k][:n] or (n == 0 and r[k] is None), k       # (an empty array may travel as NULL)
    if n:
        assert r["blocks"] == BLOCKS[:n]


# ---------------------------------------------------------------- the eight forms with caller-given output slots
@pytest.mark.parametrize("n", [3, 0])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", list(SPINE))
def test_spine_forms(lib, form, kind, n):
    symbol, middle, detail = SPINE[form]
    res, out_buf = call_spine(form, kind, n)
    assert [c["name"] for c in lib.calls] == [symbol]
    r = lib.calls[0]
    assert (r["ctx"], r["n"], r["mem_kind"], r["stream"]) == (None, n, L.MEM_HOST, None)
    check_descriptors(r, n)
    assert r["out_base"] == out_buf.ctypes.data
    assert [int(out_buf[o]) for o in OUT_OFF[:n]] == [MARK if c else 0 for c in OUT_CAP[:n]]
    check_outputs(res, n, detail)
    if "flags" in r:
        assert r["flags"] is None
    if middle == "dicts":
        assert r["ext"]["dict_base"]
        if n:
            assert r["dicts"] == DICTS[:n]
        if detail:
            assert (r["ext"]["out_pos"], r["ext"]["chain_prev"], r["ext"]["n_chains"]) == (None, None, 0)
    elif middle == "shared":
        assert (r["dict"], r["dict_len"]) == (SHARED, len(SHARED))
    elif middle == "set":
        assert r["set"] == HANDLE
        assert r["dict_id"] == IDS[:n] or (n == 0 and r["dict_id"] is None)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", ["compress_batch", "compress_batch_with_dict"])
def test_flags_given(lib, form, kind):
    res, _ = call_spine(form, kind, flags=arr(FLAGS, np.uint32, kind))
    assert lib.calls[0]["flags"] == FLAGS
    check_descriptors(lib.calls[0], 3)
    check_outputs(res, 3, False)


@pytest.mark.parametrize("form", list(SYMBOL))
def test_ctx_is_passed_on(lib, form):
    ctx = C.c_void_p(0xC7C7C7C7C7)
    if form in SPINE:
        call_spine(form, ctx=ctx)
    elif form == "decompressed_size_batch":
        block.decompressed_size_batch(u8(IN_BYTES), IN_OFF, IN_LEN, ctx=ctx)
    else:
        getattr(block, form)(u8(IN_BYTES), IN_OFF, IN_LEN, np.zeros(64, np.uint8), ctx=ctx)
    assert lib.calls[0]["ctx"] == ctx.value


@pytest.mark.parametrize("form", list(SYMBOL))
def test_an_empty_input_buffer_is_null(lib, form):
    empty, zeros = np.zeros(0, np.uint8), [0, 0, 0]
    if form in SPINE:
        middle = {"dicts": [u8(DICT_BYTES), DICT_OFF, DICT_LEN], "shared": [u8(SHARED)], "set": [IDS, the_set()], "": []}[SPINE[form][1]]
        getattr(block, form)(empty, zeros, zeros, *middle, np.zeros(80, np.uint8), OUT_OFF, OUT_CAP)
    elif form == "decompressed_size_batch":
        block.decompressed_size_batch(empty, zeros, zeros)
    else:
        getattr(block, form)(empty, zeros, zeros, np.zeros(64, np.uint8))
    r = lib.calls[0]
    assert r["in_base"] is None and r["in_len"] == zeros and r["blocks"] == [b""] * 3


@pytest.mark.parametrize("form", ["compress_batch_with_dict", "decompress_batch_with_dict"])
def test_an_empty_dictionary_buffer_still_has_an_address(lib, form):
    """NULL would mean "no dictionaries" for the whole batch: the ext structure names a buffer and the per-block arrays even so"""
    call_spine(form, dict_buf=np.zeros(0, np.uint8))
    e = lib.calls[0]["ext"]
    assert e["dict_base"] and e["dict_off"] and e["dict_len"]
    call_spine(form, dict_buf=b"")
    assert lib.calls[1]["ext"]["dict_base"]


@pytest.mark.parametrize("empty", [b"", np.zeros(0, np.uint8)])
@pytest.mark.parametrize("form", ["compress_batch_with_shared_dict", "decompress_batch_with_shared_dict"])
def test_an_empty_shared_dictionary_is_null(lib, form, empty):
    res, _ = call_spine(form, shared=empty)
    r = lib.calls[0]
    assert (r["dict"], r["dict_len"]) == (None, 0)
    check_descriptors(r, 3)
    check_outputs(res, 3, SPINE[form][2])


@pytest.mark.parametrize("ids", [[0, 1], [0, 1, 2, 0], np.zeros(0, np.uint32)])
@pytest.mark.parametrize("form", ["compress_batch_with_dict_set", "decompress_batch_with_dict_set"])
def test_dict_id_of_the_wrong_length(lib, form, ids):
    with pytest.raises(ValueError):
        call_spine(form, ids=ids)
    assert not lib.calls


def test_a_closed_set_is_refused(lib):
    s = the_set()
    s.close()
    with pytest.raises(ValueError):
        call_spine("compress_batch_with_dict_set", dict_set=s)
    assert not lib.calls


# ---------------------------------------------------------------- the size query
@pytest.mark.parametrize("n", [3, 0])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("history", [None, [0, 65536, 0xFFFFFFFF]])
def test_decompressed_size_batch(lib, kind, history, n):
    h = None if history is None else arr(history, np.uint32, kind, n)
    size, status = block.decompressed_size_batch(u8(IN_BYTES, kind), arr(IN_OFF, np.uint64, kind, n), arr(IN_LEN, np.uint32, kind, n), history=h)
    assert [c["name"] for c in lib.calls] == ["lz4flex_decompressed_size_batch"]
    r = lib.calls[0]
    assert (r["ctx"], r["n"], r["mem_kind"], r["stream"]) == (None, n, L.MEM_HOST, None)
    check_descriptors(r, n, ("in_off", "in_len"))
    assert r["history"] == (None if history is None else history[:n]) or (n == 0 and r["history"] is None)
    assert size.dtype == np.uint64 and size.shape == (n,) and size.tolist() == w_size(n)
    assert status.dtype == np.int32 and status.shape == (n,) and status.tolist() == w_status(n)


# ---------------------------------------------------------------- the packed pair
@pytest.mark.parametrize("n", [3, 0])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode,sizes", [("prepended", None), ("given", [5, 0, 70000]), ("scan", None), ("scan", [1, 2, 3])])
def test_decompress_batch_packed(lib, kind, mode, sizes, n):
    out_buf = np.zeros(64, np.uint8)
    s = None if sizes is None else arr(sizes, np.uint32, kind, n)
    res = block.decompress_batch_packed(u8(IN_BYTES, kind), arr(IN_OFF, np.uint64, kind, n), arr(IN_LEN, np.uint32, kind, n), out_buf,
                                        size_mode=mode, sizes=s)
    assert [c["name"] for c in lib.calls] == ["lz4flex_decompress_batch_packed"]
    r = lib.calls[0]
    assert (r["ctx"], r["n"], r["mem_kind"], r["stream"], r["work"]) == (None, n, L.MEM_HOST, None, None)
    assert r["size_mode"] == {"prepended": L.SIZES_PREPENDED, "given": L.SIZES_GIVEN, "scan": L.SIZES_SCAN}[mode] == block.SIZE_MODES[mode]
    check_descriptors(r, n, ("in_off", "in_len"))
    assert r["sizes"] == (None if sizes is None else sizes[:n]) or (n == 0 and r["sizes"] is None)
    assert (r["out_base"], r["total_cap"], r["align"]) == (out_buf.ctypes.data, 64, 1) and out_buf[0] == MARK
    assert len(res) == 5
    out_off, out_cap = res[:2]
    assert out_off.dtype == np.uint64 and out_off.shape == (n + 1,) and out_off.tolist() == w_packed_off(n)
    assert out_cap.dtype == np.uint32 and out_cap.shape == (n,) and out_cap.tolist() == w_packed_cap(n)
    check_outputs(res[2:], n, True)


@pytest.mark.parametrize("n", [3, 0])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("prepend", [True, False])
def test_compress_batch_packed(lib, kind, prepend, n):
    out_buf = np.zeros(64, np.uint8)
    res = block.compress_batch_packed(u8(IN_BYTES, kind), arr(IN_OFF, np.uint64, kind, n), arr(IN_LEN, np.uint32, kind, n), out_buf,
                                      prepend_size=prepend)
    assert [c["name"] for c in lib.calls] == ["lz4flex_compress_batch_packed"]
    r = lib.calls[0]
    assert (r["ctx"], r["n"], r["mem_kind"], r["stream"], r["work"]) == (None, n, L.MEM_HOST, None, None)
    check_descriptors(r, n, ("in_off", "in_len"))
    assert r["prepend_size"] == int(prepend)
    assert lib.bounds == [(sum(IN_LEN[:n]), n, int(prepend))]          # the scratch the library allocates for a host call is sized by its own bound
    assert (r["scratch"], r["scratch_cap"]) == (None, SCRATCH_BOUND)
    assert (r["out_base"], r["total_cap"], r["align"]) == (out_buf.ctypes.data, 64, 1) and out_buf[0] == MARK
    assert len(res) == 3
    assert res[0].dtype == np.uint64 and res[0].shape == (n + 1,) and res[0].tolist() == w_packed_off(n)
    check_outputs(res[1:], n, False)


@pytest.mark.parametrize("form", ["decompress_batch_packed", "compress_batch_packed"])
def test_packed_scalars(lib, form):
    f = getattr(block, form)
    out_buf = np.zeros(64, np.uint8)
    f(u8(IN_BYTES), IN_OFF, IN_LEN, out_buf, total_cap=48, align=256)
    f(u8(IN_BYTES), IN_OFF, IN_LEN, out_buf, total_cap=0)
    f(u8(IN_BYTES), IN_OFF, IN_LEN, out_buf, total_cap=(1 << 32) + 5)          # (a u64: nothing is truncated)
    f(u8(IN_BYTES), IN_OFF, IN_LEN, np.zeros(0, np.uint8))
    assert [(c["total_cap"], c["align"]) for c in lib.calls] == [(48, 256), (0, 1), ((1 << 32) + 5, 1), (0, 1)]
    assert [c["out_base"] for c in lib.calls[:3]] == [out_buf.ctypes.data] * 3 and lib.calls[3]["out_base"] is None
    if form == "decompress_batch_packed":
        f(u8(IN_BYTES), IN_OFF, IN_LEN, out_buf, big_blocks=True)
        assert lib.calls[4]["mem_kind"] == L.MEM_HOST | L.MEM_BIG_BLOCKS
        with pytest.raises(KeyError):
            f(u8(IN_BYTES), IN_OFF, IN_LEN, out_buf, size_mode="guess")
        assert len(lib.calls) == 5


# ---------------------------------------------------------------- failures
@pytest.mark.parametrize("form", list(SYMBOL))
def test_a_return_code_raises_device_error(lib, form):
    s = the_set() if form.endswith("_dict_set") else None
    lib.rc = -L.E_HIP
    with pytest.raises(block.DeviceError) as e:
        if form in SPINE:
            call_spine(form, dict_set=s)
        elif form == "decompressed_size_batch":
            block.decompressed_size_batch(u8(IN_BYTES), IN_OFF, IN_LEN)
        else:
            getattr(block, form)(u8(IN_BYTES), IN_OFF, IN_LEN, np.zeros(64, np.uint8))
    assert len(lib.calls) == 1
    text = str(e.value)
    assert SYMBOL[form] + " " in text and "(%d)" % -L.E_HIP in text and LAST_ERROR in text


def test_the_stand_in_refuses_a_wrong_argument_count(lib):
    with pytest.raises(TypeError):
        lib.lz4flex_decompress_batch(None, None, None, None, 0, None, None, None, None, None, None, L.MEM_HOST)
    with pytest.raises(TypeError):
        lib.lz4flex_decompress_batch(None, None, None, None, 0, None, None, None, None, None, None, L.MEM_HOST, None, None)
    assert lib.lz4flex_decompress_batch(None, None, None, None, 0, None, None, None, None, None, None, L.MEM_HOST, None) == 0


# ---------------------------------------------------------------- DictSet
def test_dict_set_flattens_its_dictionaries(lib):
    parts = [b"first", np.frombuffer(b"the second", np.uint8), b"", bytearray(b"4th")]
    s = block.DictSet(parts)
    assert len(lib.sets) == 1
    c = lib.sets[0]
    assert (c["ctx"], c["k"], c["mem_kind"]) == (None, 4, L.MEM_HOST)
    assert (c["off"], c["len"]) == ([0, 5, 15, 15], [5, 10, 0, 3])
    assert c["dicts"] == [b"first", b"the second", b"", b"4th"]
    assert c["flat"] == b"firstthe second4th"
    assert s.lengths.dtype == np.uint32 and s.lengths.tolist() == [5, 10, 0, 3]
    assert s.handle.value == HANDLE and len(s) == 4
    assert not lib.freed
    s.close()
    s.close()
    assert lib.freed == [HANDLE]
    with pytest.raises(ValueError):
        s.handle
    with pytest.raises(ValueError):
        len(s)
    del s
    assert lib.freed == [HANDLE]


def test_dict_set_context_manager_and_ctx(lib):
    ctx = C.c_void_p(0xABCD)
    with block.DictSet([b"only"], ctx=ctx) as s:
        assert lib.sets[0]["ctx"] == 0xABCD and s.handle.value == HANDLE
    assert lib.freed == [HANDLE]


@pytest.mark.parametrize("parts", [[], [b""], [b"", np.zeros(0, np.uint8)]])
def test_dict_set_without_bytes_still_has_an_address(lib, parts):
    s = block.DictSet(parts)
    c = lib.sets[0]
    assert c["dict_base"] and c["k"] == len(parts) and c["dicts"] == [b""] * len(parts)
    assert s.lengths.tolist() == [0] * len(parts) and len(s) == len(parts)


def test_dict_set_create_failure(lib):
    lib.rc = -L.E_NOMEM
    with pytest.raises(block.DeviceError) as e:
        block.DictSet([b"abc"])
    assert "lz4flex_dict_set_create " in str(e.value) and "(%d)" % -L.E_NOMEM in str(e.value) and LAST_ERROR in str(e.value)
    assert not lib.freed
