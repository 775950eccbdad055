"""GPU: the device (torch) forms of lz4_flex_amd.block against the host forms of the same library.

The three forms that compress into slots of the maximum output size, the three that decode raw blocks of unknown sizes and the packed
pair: what they return for an empty batch, and for one batch whose blocks lie on both sides of the two MEM_BIG_BLOCKS thresholds
(65 536 plain bytes for compressing, 131 072 for decoding) that the bytes, offsets, lengths and statuses are the host forms' -- which
the other GPU suites pin.  Bytes and integers: equal or not."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENS = [0, 13, 70000, 140000]
E_INVALID_ARG = 64


def plain(i, n):
    line = b"block %d of the batch: lz4 blocks compress repeated text well; " % i
    return (line * (n // len(line) + 1))[:n]


DICT_A = b"a dictionary that says: " + plain(2, 3000)       # block 2 begins as this dictionary ends
DICT_B = plain(3, 500) + b" -- the second dictionary"
BLOCKS = [plain(i, n) for i, n in enumerate(LENS)]


@pytest.fixture(scope="module")
def env():
    import torch
    from lz4_flex_amd import _lib, block
    assert _lib.load().lz4flex_device_count() >= 1, _lib.last_error()
    return torch, block


def layout(lens):
    lens = np.asarray(lens, np.uint64)
    return (np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint64)


def pack(blocks):
    """(bytes with one spare byte behind them, in_off, in_len)"""
    lens = np.array([len(b) for b in blocks], np.uint32)
    return np.frombuffer(b"".join(blocks) + b"\0", np.uint8).copy(), layout(lens), lens


def dev(torch, a):
    return torch.from_numpy(a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize]).copy()).to("cuda")


def host_of(torch, res):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in res]


def slots(buf, off, length):
    return [bytes(buf[int(o):int(o) + int(m)]) for o, m in zip(off, length)]


def same_as_host(got, buf, off, length, status):
    """a device form's (out, out_off, out_len, status) as numpy against a host form's buffer, layout and results, slot by slot"""
    n = len(length)
    assert got[1].view(np.uint64)[:len(off)].tolist() == [int(v) for v in off]
    assert got[2].view(np.uint32).tolist() == [int(v) for v in length]
    assert got[3].tolist() == [int(v) for v in status]
    assert slots(got[0], got[1][:n], got[2]) == slots(buf, off[:n], length)


# ---------------------------------------------------------------- the three dictionary arrangements
def ex_arrays():
    """per-block dictionaries: (dict_buf, dict_off, dict_len) -- none, B, A, none"""
    buf = np.frombuffer(b"#" + DICT_A + b"##" + DICT_B, np.uint8).copy()
    return buf, np.array([0, 3 + len(DICT_A), 1, 0], np.uint64), np.array([0, len(DICT_B), len(DICT_A), 0], np.uint32)


SET_IDS = [1, 0xFFFFFFFF, 0, 2]         # B, none, A, the set's empty dictionary


def arrangements(env):
    """name -> (compress on the device, compress on the host, decode on the device or None, decode on the host, history per block);
    every function takes the batch alone"""
    torch, block = env
    dbuf, doff, dlen = ex_arrays()
    nbuf = np.zeros(0, np.uint8)
    zero = np.zeros(4, np.uint32)
    shared = np.frombuffer(DICT_A, np.uint8).copy()
    ids = np.array(SET_IDS, np.uint32)
    the_set = block.DictSet([DICT_A, DICT_B, b""])
    t = lambda a: dev(torch, a)      # noqa: E731
    return the_set, {
        "plain": (lambda s, o, m: block.compress_blocks_with_dict_device(s, o, m, t(nbuf), t(zero.astype(np.uint64)), t(zero)),
                  lambda b, o, m, ob, oo, oc: block.compress_batch(b, o, m, ob, oo, oc),
                  lambda s, o, m: block.decompress_blocks_device(s, o, m),
                  lambda b, o, m, ob, oo, oc: block.decompress_batch(b, o, m, ob, oo, oc), None),
        "per block": (lambda s, o, m: block.compress_blocks_with_dict_device(s, o, m, t(dbuf), t(doff), t(dlen)),
                      lambda b, o, m, ob, oo, oc: block.compress_batch_with_dict(b, o, m, dbuf, doff, dlen, ob, oo, oc),
                      None,
                      lambda b, o, m, ob, oo, oc: block.decompress_batch_with_dict(b, o, m, dbuf, doff, dlen, ob, oo, oc), dlen),
        "shared": (lambda s, o, m: block.compress_blocks_with_shared_dict_device(s, o, m, t(shared)),
                   lambda b, o, m, ob, oo, oc: block.compress_batch_with_shared_dict(b, o, m, shared, ob, oo, oc),
                   lambda s, o, m: block.decompress_blocks_with_shared_dict_device(s, o, m, t(shared)),
                   lambda b, o, m, ob, oo, oc: block.decompress_batch_with_shared_dict(b, o, m, shared, ob, oo, oc),
                   np.full(4, len(shared), np.uint32)),
        "set": (lambda s, o, m: block.compress_blocks_with_dict_set_device(s, o, m, t(ids), the_set),
                lambda b, o, m, ob, oo, oc: block.compress_batch_with_dict_set(b, o, m, ids, the_set, ob, oo, oc),
                lambda s, o, m: block.decompress_blocks_with_dict_set_device(s, o, m, t(ids), the_set),
                lambda b, o, m, ob, oo, oc: block.decompress_batch_with_dict_set(b, o, m, ids, the_set, ob, oo, oc),
                np.array([len(DICT_B), 0, len(DICT_A), 0], np.uint32)),
    }


@pytest.fixture(scope="module")
def forms(env):
    the_set, table = arrangements(env)
    yield table
    env[0].cuda.synchronize()
    the_set.close()


@pytest.fixture(scope="module")
def compressed(env, forms):
    """name -> the device compress form's (out, out_off, out_len, status) as device tensors, computed once"""
    torch = env[0]
    buf, off, lens = pack(BLOCKS)
    return {name: f[0](dev(torch, buf), dev(torch, off), dev(torch, lens)) for name, f in forms.items()}


# ---------------------------------------------------------------- nothing to do
def check_empty(torch, res, shapes):
    assert len(res) == 4
    for t, (dtype, shape) in zip(res, shapes):
        assert t.dtype == dtype and tuple(t.shape) == shape and t.device.type == "cuda", (t.dtype, t.shape, t.device)


def test_empty_batches(env):
    torch, block = env
    src = torch.zeros(16, dtype=torch.uint8, device="cuda")
    none = torch.zeros(0, dtype=torch.int64)
    u8 = torch.zeros(0, dtype=torch.uint8, device="cuda")
    slot_forms = [(torch.uint8, (0,)), (torch.int64, (0,)), (torch.int32, (0,)), (torch.int32, (0,))]
    with block.DictSet([b"abc"]) as s:
        for res in (block.compress_blocks_with_dict_device(src, none, none, u8, none, none),
                    block.compress_blocks_with_shared_dict_device(src, none, none, u8),
                    block.compress_blocks_with_dict_set_device(src, none, none, none, s),
                    block.decompress_blocks_device(src, none, none),
                    block.decompress_blocks_with_shared_dict_device(src, none, none, u8),
                    block.decompress_blocks_with_dict_set_device(src, none, none, none, s)):
            check_empty(torch, res, slot_forms)
    for capacity in (0, 48):
        packed = [(torch.uint8, (capacity,)), (torch.int64, (1,)), (torch.int32, (0,)), (torch.int32, (0,))]
        for res in (block.compress_blocks_packed_device(src, none, none, capacity), block.decompress_blocks_packed_device(src, none, none, capacity)):
            check_empty(torch, res, packed)
            assert res[1].tolist() == [0]


# ---------------------------------------------------------------- compress: the device form == the host form
@pytest.mark.parametrize("name", ["plain", "per block", "shared", "set"])
def test_compress_equals_the_host_form(env, forms, compressed, name):
    torch, block = env
    buf, off, lens = pack(BLOCKS)
    caps = np.array([block.get_maximum_output_size(n) for n in LENS], np.uint32)
    out_off = layout(caps)
    out_buf = np.zeros(int(caps.sum()), np.uint8)
    out_len, status = forms[name][1](buf, off, lens, out_buf, out_off, caps)
    assert (status == 0).all()
    got = host_of(torch, compressed[name])
    assert len(got[0]) == int(caps.sum())
    same_as_host(got, out_buf, out_off, out_len, status)
    # and the host decoder returns the blocks
    back = np.zeros(sum(LENS) + 1, np.uint8)
    rl, rs, _ = forms[name][3](got[0], got[1].view(np.uint64), got[2].view(np.uint32), back, off, lens)
    assert (rs == 0).all() and slots(back, off, rl) == BLOCKS


# ---------------------------------------------------------------- decode: round trip, and the device form == the host form
@pytest.mark.parametrize("name", ["plain", "shared", "set"])
def test_decode_round_trips_and_equals_the_host_form(env, forms, compressed, name):
    torch, block = env
    comp, c_off, c_len, _ = compressed[name]
    got = host_of(torch, forms[name][2](comp, c_off, c_len))
    assert got[3].tolist() == [0] * 4 and len(got[0]) == sum(LENS)
    assert slots(got[0], got[1], got[2]) == BLOCKS
    _, off, lens = pack(BLOCKS)
    back = np.zeros(sum(LENS) + 1, np.uint8)
    h = host_of(torch, [comp, c_off, c_len])
    rl, rs, _ = forms[name][3](h[0], h[1].view(np.uint64), h[2].view(np.uint32), back, off, lens)
    same_as_host(got, back, off, rl, rs)


@pytest.mark.parametrize("name", ["plain", "shared", "set"])
def test_decode_with_one_block_cut(env, forms, compressed, name):
    """the last byte of block 2 is missing: the block has the size pass's status and an empty slot, its neighbours are whole"""
    torch, block = env
    comp, c_off, c_len, _ = compressed[name]
    cut = c_len.clone()
    cut[2] -= 1
    h = host_of(torch, [comp, c_off, cut])
    size, size_status = block.decompressed_size_batch(h[0], h[1].view(np.uint64), h[2].view(np.uint32), history=forms[name][4])
    assert size_status[2] != 0 and size_status.tolist().count(0) == 3 and size.tolist() == [LENS[0], LENS[1], 0, LENS[3]]
    got = host_of(torch, forms[name][2](comp, c_off, cut))
    assert got[3].tolist() == size_status.tolist()
    assert got[1].tolist() == layout(size).tolist() and got[2].tolist() == size.tolist() and len(got[0]) == int(size.sum())
    assert slots(got[0], got[1], got[2]) == [BLOCKS[0], BLOCKS[1], b"", BLOCKS[3]]


def test_an_id_the_set_does_not_have_is_the_decoders_to_report(env, forms, compressed):
    """block 2 was compressed against dictionary 0 and reaches into it: with an id >= k it has no history, the size pass rejects it --
    and the decoder's E_INVALID_ARG is the status it gets"""
    torch, block = env
    comp, c_off, c_len, _ = compressed["set"]
    h = host_of(torch, [comp, c_off, c_len])
    history = forms["set"][4].copy()
    history[2] = 0
    size, size_status = block.decompressed_size_batch(h[0], h[1].view(np.uint64), h[2].view(np.uint32), history=history)
    assert size_status[2] not in (0, E_INVALID_ARG), "the case does not reach the merge rule's exception"
    ids = torch.tensor([1, 0xFFFFFFFF, 3, 2], dtype=torch.int64)
    with block.DictSet([DICT_A, DICT_B, b""]) as s:
        got = host_of(torch, block.decompress_blocks_with_dict_set_device(comp, c_off, c_len, ids, s))
    assert got[3].tolist() == [0, 0, E_INVALID_ARG, 0]
    assert got[2].tolist() == [LENS[0], LENS[1], 0, LENS[3]] and got[1].tolist() == layout(size).tolist()
    assert slots(got[0], got[1], got[2]) == [BLOCKS[0], BLOCKS[1], b"", BLOCKS[3]]


# ---------------------------------------------------------------- the packed pair
def test_packed_forms_equal_the_host_forms(env):
    torch, block = env
    buf, off, lens = pack(BLOCKS)
    capacity = sum(block.get_maximum_output_size(n) + 4 for n in LENS)
    comp = block.compress_blocks_packed_device(dev(torch, buf), dev(torch, off), dev(torch, lens), capacity, big_blocks=True)
    got = host_of(torch, comp)
    h_buf = np.zeros(capacity, np.uint8)
    h_off, h_len, h_status = block.compress_batch_packed(buf, off, lens, h_buf)
    assert (h_status == 0).all() and len(got[0]) == capacity
    same_as_host(got, h_buf, h_off, h_len, h_status)
    room = sum(LENS) + 64
    out = host_of(torch, block.decompress_blocks_packed_device(comp[0], comp[1][:4], comp[2], room, align=16, big_blocks=True))
    assert out[3].tolist() == [0] * 4 and len(out[0]) == room
    assert slots(out[0], out[1][:4], out[2]) == BLOCKS
    r_buf = np.zeros(room, np.uint8)
    r_off, _r_cap, r_len, r_status, _ = block.decompress_batch_packed(h_buf, h_off[:4], h_len, r_buf, align=16, big_blocks=True)
    same_as_host(out, r_buf, r_off, r_len, r_status)
