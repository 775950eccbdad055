"""GPU (-m gpu): the throughput encoder places window k's segments while window k + 1 is matched (lz4_compress_wave.hip,
resolve_window / copy_segment): the sizes are resolved behind the matching barrier, the bytes are copied a window later by whichever
worker is done first, from the window's record in LDS and from body set k & 1.

What can go wrong is order and reuse -- a record or a body set read after the next window has overwritten it, a skipped item or an
empty batch tail between two deferred windows, the last window of a workgroup, a block's last window followed by another block's
first, literals fetched when the staging slot already holds the next window, a launch that starts while the one before still copies.
Every case: device-resident batch, every block's bytes / out_len / status == the scalar model (tests/sim/wave_encoder_model.c
through wave_model), and the 0xEE canary behind every block's out_cap untouched."""
import ctypes as C

import numpy as np
import pytest

import corpus
import dict_cases as D
import oracle_api as O
import wave_model as W

pytestmark = pytest.mark.gpu

CANARY = 0xEE
PAD = 64
LENS = [0, 1, 12, 13, 64, 700, 4096, 9000]


def _L():
    from lz4_flex_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def lib():
    L = _L()
    lib = L.load()
    assert lib.lz4flex_device_count() >= 1
    assert lib.lz4flex_set_tuning(None, b"compress_mode", 0) == 0     # the throughput encoder on the default context
    return lib


@pytest.fixture(scope="module")
def G(lib):
    g = lib.lz4flex_get_tuning(None, b"compress_workgroups")
    assert g >= 2
    return g


class tuning:
    """settings of the default context, restored on the way out"""
    DEFAULTS = {b"compress_subwindows": 0, b"compress_carry_wait": 1, b"compress_sliding_window": W.SLIDE_DEFAULT}

    def __init__(self, lib, **kw):
        self.lib, self.kw = lib, {k.encode(): v for k, v in kw.items()}

    def __enter__(self):
        for k, v in self.kw.items():
            assert self.lib.lz4flex_set_tuning(None, k, v) == 0
        return self

    def __exit__(self, *exc):
        for k in self.kw:
            assert self.lib.lz4flex_set_tuning(None, k, self.DEFAULTS[k]) == 0
        return False


_source = None


def source():
    """JSON, text, and the reference's round-trip strings, one after the other"""
    global _source
    if _source is None:
        _source = (O.fixture_plain("compression_66k_JSON") + O.fixture_plain("compression_65k") +
                   b"".join(bytes(s) for s in corpus.ROUNDTRIP_STRINGS)) * 2
    return _source


_blocks = {}
_model = {}


def small_blocks(n):
    """block i of every batch: length LENS[i % 8] (every 97th: a full window, all eleven segments non-empty), cut from source() at
    a phase of its own.  One list, a batch of n blocks is its first n."""
    if not _blocks.get("small") or len(_blocks["small"]) < n:
        src = source()
        half = len(src) // 2
        out = []
        for i in range(n):
            m = 65536 if i % 97 == 96 else LENS[i % len(LENS)]
            ph = (i * 7919) % half
            out.append(src[ph:ph + m])
        _blocks["small"] = out
    return _blocks["small"][:n]


def model(b, **kw):
    """wave_model.compress, once per distinct input"""
    key = (b, tuple(sorted(kw.items())))
    if key not in _model:
        _model[key] = W.compress(b, **kw)
    return _model[key]


def launch(lib, blocks, caps=None, flags=None, dicts=None, big=False, in_buf=None, in_off=None):
    """one lz4flex_compress_batch(_ex) on the current stream, device memory, not synchronised; in_buf / in_off: the blocks lie in a
    buffer of the caller's (history); dicts: (buffer, offsets, lengths)"""
    import torch
    L = _L()
    dev = torch.device("cuda", 0)
    n = len(blocks)
    if in_buf is None:
        in_off, pos = [], 1
        for b in blocks:
            in_off.append(pos)
            pos += len(b) + 3                                            # unaligned block starts
        in_buf = np.zeros(pos + 64, np.uint8)
        for o, b in zip(in_off, blocks):
            in_buf[o:o + len(b)] = np.frombuffer(b, np.uint8)
    caps = [O.max_out(len(b)) for b in blocks] if caps is None else list(caps)
    out_off, pos = [], 5
    for c in caps:
        out_off.append(pos)
        pos += c + PAD
    i64 = lambda v: torch.tensor(np.array(v, np.uint64).view(np.int64), device=dev)      # noqa: E731
    i32 = lambda v: torch.tensor(np.array(v, np.uint32).view(np.int32), device=dev)      # noqa: E731
    t = dict(in_buf=torch.from_numpy(np.array(in_buf, dtype=np.uint8)).to(dev), in_off=i64(in_off), in_len=i32([len(b) for b in blocks]),
             out_buf=torch.full((pos,), CANARY, dtype=torch.uint8, device=dev), out_off=i64(out_off), out_cap=i32(caps),
             out_len=torch.full((n,), -7, dtype=torch.int32, device=dev), status=torch.full((n,), -7, dtype=torch.int32, device=dev))
    if flags is not None:
        t["flags"] = i32(flags)
    p = lambda x: C.c_void_p(x.data_ptr())                                # noqa: E731
    mem = L.MEM_DEVICE | (L.MEM_BIG_BLOCKS if big else 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fl = p(t["flags"]) if flags is not None else None
    if dicts is not None:
        t["dict_buf"] = torch.from_numpy(np.array(dicts[0], dtype=np.uint8)).to(dev)
        t["dict_off"], t["dict_len"] = i64(dicts[1]), i32(dicts[2])
        e = L.CompressExt(t["dict_buf"].data_ptr(), t["dict_off"].data_ptr(), t["dict_len"].data_ptr())
        rc = lib.lz4flex_compress_batch_ex(None, p(t["in_buf"]), p(t["in_off"]), p(t["in_len"]), fl, n, p(t["out_buf"]), p(t["out_off"]),
                                           p(t["out_cap"]), p(t["out_len"]), p(t["status"]), C.byref(e), mem, stream)
    else:
        rc = lib.lz4flex_compress_batch(None, p(t["in_buf"]), p(t["in_off"]), p(t["in_len"]), fl, n, p(t["out_buf"]), p(t["out_off"]),
                                        p(t["out_cap"]), p(t["out_len"]), p(t["status"]), mem, stream)
    assert rc == 0, (rc, L.last_error())
    return dict(t=t, out_off=out_off, caps=caps, n=n)


def collect(h):
    """(outputs, out_len, status) of a launch, after the device is done; the canary behind every out_cap, and the whole sink of a
    block that reports an error, must be untouched"""
    import torch
    torch.cuda.synchronize()
    out_buf = h["t"]["out_buf"].cpu().numpy()
    out_len = h["t"]["out_len"].cpu().numpy().view(np.uint32)
    status = h["t"]["status"].cpu().numpy()
    outs = []
    for i in range(h["n"]):
        o, c = h["out_off"][i], h["caps"][i]
        assert (out_buf[o + c:o + c + PAD] == CANARY).all(), "block %d wrote behind its out_cap" % i
        if status[i] != 0:
            assert out_len[i] == 0, i
            assert (out_buf[o:o + c] == CANARY).all(), "block %d (status %d) wrote bytes" % (i, status[i])
        else:
            assert out_len[i] <= c, i
        outs.append(bytes(out_buf[o:o + int(out_len[i])]))
    return outs, out_len, status


def check_equal(outs, out_len, status, want, skip=()):
    bad = [(i, int(status[i]), int(out_len[i]), len(want[i])) for i in range(len(want))
           if i not in skip and (status[i] != 0 or int(out_len[i]) != len(want[i]) or outs[i] != want[i])]
    assert not bad, bad[:8]


def batch_sizes(G):
    return [1, G - 1, G, G + 1, 2 * G, 2 * G + 1, 3 * G + 1]


@pytest.mark.parametrize("which", range(7))
def test_one_two_three_windows_per_workgroup(lib, G, which):
    """1 ... 3G + 1 one-window blocks (compress_subwindows 1): a workgroup has one, two, three or four windows, so body set and record
    parity 0 and 1 are used zero to two times, with prologue and epilogue; below G blocks the windows are dealt out (window mode)"""
    n = batch_sizes(G)[which]
    blocks = small_blocks(n)
    want = [model(b, sub=1) for b in blocks]
    with tuning(lib, compress_subwindows=1):
        outs, ol, st = collect(launch(lib, blocks))
    check_equal(outs, ol, st, want)
    assert O.decompress(outs[n - 1], len(blocks[n - 1])) == ("ok", blocks[n - 1])


def test_skipped_items_between_deferred_ones(lib, G):
    """out_cap too small for every block i = 3 (mod 5): OutputTooSmall and out_len 0, nothing written, no tickets for that window; the
    blocks the same workgroup encodes a window earlier and later (i - G, i + G) and all others are what they are without"""
    L = _L()
    n = 3 * G + 1
    blocks = small_blocks(n)
    want = [model(b, sub=1) for b in blocks]
    caps = [O.max_out(len(b)) - (1 if i % 5 == 3 else 0) for i, b in enumerate(blocks)]
    with tuning(lib, compress_subwindows=1):
        outs, ol, st = collect(launch(lib, blocks, caps=caps))
    small = [i for i in range(n) if i % 5 == 3]
    assert all(st[i] == L.E_OUTPUT_TOO_SMALL and ol[i] == 0 for i in small)
    check_equal(outs, ol, st, want, skip=set(small))
    for i in small:
        for k in (i - G, i + G):
            if 0 <= k < n and k % 5 != 3:
                assert st[k] == 0 and outs[k] == want[k], (i, k)


def test_run_windows_next_to_ordinary_ones(lib, G):
    """blocks of 8 192, 40 000 and 65 536 equal bytes at indices j and j + G (one workgroup: run window, run window, text), text blocks
    around them: a run window's single segment goes through the same record and the same tickets"""
    n = 3 * G + 1
    txt = O.fixture_plain("compression_65k")
    blocks = [txt[(i % 13) * 997:(i % 13) * 997 + [700, 4096, 9000][i % 3]] for i in range(n)]
    for m, size in enumerate((8192, 40000, 65536)):
        blocks[1 + m] = bytes([0x11 * (m + 1)]) * size
        blocks[1 + m + G] = bytes(size)
    want = [model(b, sub=1) for b in blocks]
    assert len(want[3]) < 300                                             # (one sequence: it is a run window)
    with tuning(lib, compress_subwindows=1):
        outs, ol, st = collect(launch(lib, blocks))
    check_equal(outs, ol, st, want)


def long_blocks(k):
    src = source()
    n = 5 * 65536 + 123
    return [(src[1000 * (i + 1):] + src)[:n] for i in range(k)]


@pytest.mark.parametrize("carry_wait", [1, 0])
def test_window_mode_carry_resolved_bytes_copied_later(lib, carry_wait):
    """three blocks of 5 x 65 536 + 123 bytes (LZ4FLEX_MEM_BIG_BLOCKS), their windows dealt to the workgroups: the carry is resolved and
    handed on at the barrier, the bytes are copied a window later; a workgroup goes from a block's last window to another's first.
    carry_wait 0: every window that has to wait gives up, the second launch encodes the block again"""
    blocks = long_blocks(3)
    want = [model(b) for b in blocks]
    with tuning(lib, compress_carry_wait=carry_wait):
        outs, ol, st = collect(launch(lib, blocks, big=True))
    check_equal(outs, ol, st, want)
    assert O.decompress(outs[0], len(blocks[0])) == ("ok", blocks[0])


def test_window_mode_without_sliding_windows(lib):
    blocks = long_blocks(2)
    want = [model(b, slide=0) for b in blocks]
    with tuning(lib, compress_sliding_window=0):
        outs, ol, st = collect(launch(lib, blocks, big=True))
    check_equal(outs, ol, st, want)


def test_history_batch(lib, G):
    """LZ4FLEX_BLOCK_HISTORY, 2G + 1 small blocks cut from one stream, each with the 32 KiB in front of it as history: the model's
    history form, as in test_gpu_wave_encoder.py"""
    n = 2 * G + 1
    src = source()
    lens = [LENS[1 + i % (len(LENS) - 1)] for i in range(n)]
    stream = (src * ((W.HIST + sum(lens)) // len(src) + 2))[:W.HIST + sum(lens)]
    in_off = [W.HIST + int(x) for x in np.concatenate([[0], np.cumsum(lens)[:-1]])]
    blocks = [stream[o:o + m] for o, m in zip(in_off, lens)]
    want = [model(stream[o - W.HIST:o + m], hist=W.HIST) for o, m in zip(in_off, lens)]
    buf = np.frombuffer(stream + bytes(64), np.uint8)
    with tuning(lib, compress_subwindows=1):
        outs, ol, st = collect(launch(lib, blocks, flags=[W.HIST << 8] * n, in_buf=buf, in_off=in_off))
    check_equal(outs, ol, st, want)
    k = n - 2
    assert O.decompress(outs[k], lens[k], dict_data=stream[in_off[k] - W.HIST:in_off[k]]) == ("ok", blocks[k])


def test_dictionary_batch(lib, G):
    """lz4flex_compress_batch_ex, 2G + 1 small blocks with per-block dictionaries of three lengths: the literals come from the input
    while the staging slot already holds the next window; the model's dictionary form, as in test_gpu_compress_dict.py"""
    n = 2 * G + 1
    dsrc = D.stream("json", 50000, 0)
    dl = [100, 4096, 40000]
    dict_buf = np.frombuffer(dsrc, np.uint8)
    blocks = [D.block("json", LENS[i % len(LENS)], salt=i % 29) for i in range(n)]
    doff = [len(dsrc) - dl[i % 3] for i in range(n)]
    dlen = [dl[i % 3] for i in range(n)]
    cache = {}
    want = []
    for i, b in enumerate(blocks):
        key = (b, i % 3)
        if key not in cache:
            cache[key] = D.model(b, dsrc[doff[i]:])
        want.append(cache[key])
    with tuning(lib, compress_subwindows=1):
        outs, ol, st = collect(launch(lib, blocks, dicts=(dict_buf, doff, dlen)))
    check_equal(outs, ol, st, want)
    assert D.oracle_decodes(outs[5], blocks[5], dsrc[doff[5]:])


def test_two_launches_back_to_back(lib, G):
    """two batches on one context and stream, no synchronise between them: the second launch's first windows reuse the body sets and the
    workspace the first launch's last copies read"""
    n = 2 * G + 1
    a = small_blocks(n)
    b = list(reversed(small_blocks(3 * G + 1)))[:n]
    with tuning(lib, compress_subwindows=1):
        ha = launch(lib, a)
        hb = launch(lib, b)
        ra, rb = collect(ha), collect(hb)
    check_equal(*ra, [model(x, sub=1) for x in a])
    check_equal(*rb, [model(x, sub=1) for x in b])
