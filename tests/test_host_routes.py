"""lz4_flex_amd/csrc/lz4_route.h on the CPU: which decoder, geometry, pair mode and second pass a decode batch takes (decode_route),
which encoder a compress call takes (encode_route), and the tables the "decompress_variant" check and the "decoder_config_<i>" /
"dispatch_threshold_<i>" lists are read off.

The expected tables never come from the header: they are written here by hand from the rule (the issue text restated in DESIGN.md 5.2
"Dispatch" and 5.3a), the "decompress_variant" paragraph of include/lz4flex_amd.h (7 a workgroup per block, 8 its test geometry, 10 / 11
with 256 / 512 lanes: what 0 picks for 513 ... 640 / 257 ... 512 blocks; 13 what 0 picks for 641 ... 14 336 blocks; 4 above; 9 and 12
in tools builds; 5 and 6 gone) and the six dispatch thresholds 128, 256, 512, 640, 14 336, 16 384.

A route is (decoder, workgroup geometry, pair, redo): decoder REF / SPLIT / WG / PLAN / FUSED / SEQ = 1 / 4 / 7 / 9 / 12 / 13, geometry 0
(1 024 lanes) / 1 (tests) / 2 (256 lanes) / 3 (512 lanes), redo NONE / BATCH / CHAIN."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sim", "host_routes_shim.cpp")
HDR = os.path.join(ROOT, "lz4_flex_amd", "csrc", "lz4_route.h")
SO = os.path.join(ROOT, "tests", "sim", "libhost_routes_shim.so")

REF, SPLIT, WG, PLAN, FUSED, SEQ = 1, 4, 7, 9, 12, 13
NONE, BATCH, CHAIN = 0, 1, 2
THRESHOLDS = [128, 256, 512, 640, 14336, 16384]
CONFIGS = [1016, 4008, 4032, 4064, 7000, 8000, 10000, 11000, 13000]
CONFIGS_TOOLS = CONFIGS + [9000, 12000]
VARIANTS = {0, 1, 4, 7, 8, 10, 11, 13}
VARIANTS_TOOLS = VARIANTS | {9, 12}

_m = None


def shim():
    global _m
    if _m is None:
        if not os.path.exists(SO) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(SO):
            subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-Wall", SRC, "-o", SO])
        m = C.CDLL(SO)
        m.hr_decode_route.restype = None
        m.hr_decode_route.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        m.hr_encode_route.restype = None
        m.hr_encode_route.argtypes = [C.POINTER(C.c_int)] * 3
        m.hr_chain_max_blocks.restype = C.c_uint32
        _m = m
    return _m


def decode(n, variant=0, big=False, prefix=False, chained=False, chain_prev=False, n_chains=0, block_dicts=False, dict_source=False,
           partial=False, pcd_pair=1, shared=1, partial_on=1, pair_ws=True, tools=False, plan_fits=True):
    st = (C.c_int * 7)(variant, pcd_pair, shared, partial_on, pair_ws, tools, plan_fits)
    sh = (C.c_uint32 * 9)(n, big, prefix, chained, chain_prev, n_chains, block_dicts, dict_source, partial)
    out = (C.c_int * 4)()
    shim().hr_decode_route(st, sh, out)
    return tuple(out)


def encode(mode, high_dict, high_linked, dicts, flags, linked):
    out = (C.c_int * 2)()
    shim().hr_encode_route((C.c_int * 3)(mode, high_dict, high_linked), (C.c_int * 3)(dicts, flags, linked), out)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- decode, plain form
# n -> (decoder, geometry, redo) of "decompress_variant" 0 for blocks not known to be large, no prefix: every threshold and its successor
AUTO = {
    0: (WG, 0, BATCH), 1: (WG, 0, BATCH),
    128: (WG, 0, BATCH), 129: (WG, 0, BATCH),
    256: (WG, 0, BATCH), 257: (WG, 3, BATCH),
    512: (WG, 3, BATCH), 513: (WG, 2, BATCH),
    640: (WG, 2, BATCH), 641: (SEQ, 0, BATCH),
    14336: (SEQ, 0, BATCH), 14337: (SPLIT, 0, NONE),
    16384: (SPLIT, 0, NONE), 16385: (SPLIT, 0, NONE),
}


def test_auto_route_at_every_threshold():
    assert sorted(set(AUTO) - {0, 1}) == sorted(THRESHOLDS + [t + 1 for t in THRESHOLDS])
    for n, (dec, geo, redo) in AUTO.items():
        assert decode(n) == (dec, geo, False, redo), n
        # blocks known to be large: a full workgroup each at any count; two workgroups each up to 128 blocks ("decompress_pcd_pair" 1)
        assert decode(n, big=True) == (WG, 0, n <= 128, BATCH), n


# variant -> (decoder, geometry, redo): a batch without prefix and chain | with a prefix, not chained | a chain.  9 and 12: tools builds.
PINNED = {
    1: ((REF, 0, NONE), (REF, 0, NONE), (WG, 0, CHAIN)),               # (the reference's order has no chained form)
    4: ((SPLIT, 0, NONE), (WG, 0, BATCH), (WG, 0, CHAIN)),
    7: ((WG, 0, BATCH), (WG, 0, BATCH), (WG, 0, CHAIN)),
    8: ((WG, 1, BATCH), (WG, 1, BATCH), (WG, 1, CHAIN)),
    9: ((PLAN, 0, BATCH), (WG, 0, BATCH), (WG, 0, CHAIN)),
    10: ((WG, 2, BATCH), (WG, 2, BATCH), (WG, 2, CHAIN)),               # (an explicit geometry holds behind the rewrite to 7)
    11: ((WG, 3, BATCH), (WG, 3, BATCH), (WG, 3, CHAIN)),
    12: ((FUSED, 0, BATCH), (WG, 0, BATCH), (WG, 0, CHAIN)),
    13: ((SEQ, 0, BATCH), (SEQ, 0, BATCH), (WG, 0, CHAIN)),             # (prefixes that are in memory already: the sequence decoder keeps them)
}


@pytest.mark.parametrize("n", [1, 300, 600, 20000])
@pytest.mark.parametrize("variant", sorted(PINNED))
def test_pinned_variants_and_their_prefix_and_chain_rewrites(variant, n):
    assert set(PINNED) == VARIANTS_TOOLS - {0}
    tools = variant in (9, 12)
    plain, prefix, chain = PINNED[variant]
    for big in (False, True):
        kw = dict(variant=variant, big=big, tools=tools, pcd_pair=0)
        assert decode(n, **kw) == (plain[0], plain[1], False, plain[2])
        assert decode(n, prefix=True, **kw) == (prefix[0], prefix[1], False, prefix[2])
        assert decode(n, prefix=True, chained=True, **kw) == (chain[0], chain[1], False, chain[2])
        assert decode(n, prefix=True, chained=True, chain_prev=True, n_chains=513, **kw) == (chain[0], chain[1], False, chain[2])
        # per-block dictionaries: the reference's order whatever is pinned
        assert decode(n, block_dicts=True, **kw) == decode(n, block_dicts=True, prefix=True, **kw) == (REF, 0, False, NONE)


def test_what_a_build_has_no_kernel_for_is_the_split_decoders():
    """the product library refuses 9 and 12 (and every build 5 and 6) as a setting; LZ4FLEX_DECOMPRESS_VARIANT can still pin 5, 6 and 12
    there.  Such a batch has always fallen through to the split decoder, a prefix batch to the workgroup decoder.  A plan / replay batch
    whose plans are not addressable is the split decoder's too."""
    for v in (5, 6, 9, 12):
        assert decode(300, variant=v, tools=False) == (SPLIT, 0, False, NONE)
        assert decode(300, variant=v, tools=False, prefix=True, pcd_pair=0) == (WG, 0, False, BATCH)
    for v in (5, 6):
        assert decode(300, variant=v, tools=True) == (SPLIT, 0, False, NONE)
    assert decode(300, variant=9, tools=True, plan_fits=True) == (PLAN, 0, False, BATCH)
    assert decode(300, variant=9, tools=True, plan_fits=False) == (SPLIT, 0, False, NONE)
    assert decode(300, variant=12, tools=True, plan_fits=False) == (FUSED, 0, False, BATCH)


def test_geometry_by_the_number_of_chains():
    """several chains side by side: the chains fill the chip, so their count picks the workgroup size -- by batch shape only"""
    want = {0: 0, 256: 0, 257: 3, 512: 3, 513: 2}
    for n in (300, 1000, 20000):
        for nc, geo in want.items():
            assert decode(n, prefix=True, chained=True, chain_prev=True, n_chains=nc) == (WG, geo, False, CHAIN), (n, nc)
            assert decode(n, prefix=True, chained=True, chain_prev=False, n_chains=nc) == (WG, 0, False, CHAIN), (n, nc)
            assert decode(n, variant=7, prefix=True, chained=True, chain_prev=True, n_chains=nc) == (WG, 0, False, CHAIN), (n, nc)
    # a prefix batch keeps the full workgroup at the sizes at which a plain one gets a smaller one; an empty batch is no chain
    assert decode(300, prefix=True) == (WG, 0, False, BATCH) and decode(300) == (WG, 3, False, BATCH)
    assert decode(0, prefix=True, chained=True, chain_prev=True, n_chains=513) == (WG, 0, False, BATCH)
    assert decode(0, variant=13, prefix=True, chained=True) == (SEQ, 0, False, BATCH)
    assert decode(0, variant=1, prefix=True, chained=True) == (WG, 0, False, BATCH)


# ("decompress_pcd_pair", blocks known to be large) -> two workgroups per block, given a workspace and at most 128 blocks
PAIR = {(0, False): False, (0, True): False, (1, False): False, (1, True): True, (2, False): True, (2, True): True}


def test_pair_mode():
    for (pp, big), want in PAIR.items():
        for n, fits in ((128, True), (129, False)):
            for variant, geo in ((0, 0), (7, 0), (8, 1)):
                assert decode(n, variant=variant, big=big, pcd_pair=pp) == (WG, geo, want and fits, BATCH), (pp, big, n, variant)
                assert decode(n, variant=variant, big=big, pcd_pair=pp, pair_ws=False) == (WG, geo, False, BATCH)
                assert decode(n, variant=variant, big=big, pcd_pair=pp, prefix=True, chained=True) == (WG, geo, want and fits, CHAIN)
            # 10 and 11 are not 7: no pair -- until a prefix has rewritten them to 7, which keeps their geometry
            for variant, geo in ((10, 2), (11, 3)):
                assert decode(n, variant=variant, big=big, pcd_pair=pp) == (WG, geo, False, BATCH)
                assert decode(n, variant=variant, big=big, pcd_pair=pp, prefix=True) == (WG, geo, want and fits, BATCH), (pp, big, n, variant)
            assert decode(n, variant=4, big=big, pcd_pair=pp, prefix=True) == (WG, 0, want and fits, BATCH)
            assert decode(n, variant=13, big=big, pcd_pair=pp) == decode(n, variant=13, big=big, pcd_pair=pp, prefix=True) == (SEQ, 0, False, BATCH)
            assert decode(n, variant=4, big=big, pcd_pair=pp) == (SPLIT, 0, False, NONE)


# ---------------------------------------------------------------------------------------------------------------- decode, the six forms
ENTRIES = ["plain", "shared_dict", "dict_set", "partial", "partial_shared_dict", "partial_dict_set"]
# 1: the entry's first-pass decoder runs (and the reference-order kernel behind it); 0: the reference-order kernel decodes every block
FIRST_PASS = {
    #                           plain  shared_dict  dict_set  partial  partial_shared_dict  partial_dict_set
    "default":                  (1,    1,           1,        1,       1,                   1),
    "decompress_variant 1":     (0,    0,           0,        0,       0,                   0),
    "decompress_shared_dict 0": (1,    0,           0,        1,       0,                   0),
    "decompress_partial 0":     (1,    1,           1,        0,       0,                   0),
}
ROWS = {"default": {}, "decompress_variant 1": dict(variant=1), "decompress_shared_dict 0": dict(shared=0), "decompress_partial 0": dict(partial_on=0)}


def test_the_six_forms():
    """tests/test_gpu_decode_form_routes.py pins this table from outside on the device, with batches of at most six blocks"""
    import test_gpu_decode_form_routes as G
    assert G.FIRST_PASS == FIRST_PASS and G.ENTRIES == ENTRIES
    for row, firsts in FIRST_PASS.items():
        for entry, first in zip(ENTRIES, firsts):
            form = dict(dict_source=entry not in ("plain", "partial"), partial=entry.startswith("partial"))
            for n, plain_first in ((6, (WG, 0, False, BATCH)), (641, (SEQ, 0, False, BATCH)), (20000, (SPLIT, 0, False, NONE))):
                got = decode(n, **form, **ROWS[row])
                if entry == "plain":
                    # (the plain entry's first pass goes by batch shape; at the GPU test's six blocks it is the workgroup decoder)
                    assert got == (plain_first if first else (REF, 0, False, NONE)), (row, n)
                else:
                    # the sequence decoder at every n, whatever else is pinned
                    assert got == ((SEQ, 0, False, BATCH) if first else (REF, 0, False, NONE)), (row, entry, n)
                    if first:
                        for v in (4, 7, 8, 10, 11, 13):
                            assert decode(n, variant=v, big=True, pcd_pair=2, **form) == (SEQ, 0, False, BATCH), (entry, v)


# ---------------------------------------------------------------------------------------------------------------- encode
PLAIN, DICT, HISTORY = 0, 1, 2
# "compress_mode" 2: (dictionaries, flag words, a Linked frame's blocks) -> route under ("compress_high_dict", "compress_high_linked") =
#                                  (0, 0)       (1, 0)       (0, 1)         (1, 1)
HIGH = {
    (False, False, False):        ((2, PLAIN), (2, PLAIN), (2, PLAIN),   (2, PLAIN)),
    (False, True, False):         ((2, PLAIN), (2, PLAIN), (2, HISTORY), (2, HISTORY)),    # a direct caller's history bits: ignored or read
    (True, False, False):         ((0, PLAIN), (2, DICT),  (0, PLAIN),   (2, DICT)),
    (True, True, False):          ((0, PLAIN), (2, DICT),  (0, PLAIN),   (2, DICT)),
    # the Linked-frame rows: without "compress_high_linked" the throughput encoder, which reads the history bits
    (False, False, True):         ((0, PLAIN), (0, PLAIN), (2, PLAIN),   (2, PLAIN)),
    (False, True, True):          ((0, PLAIN), (0, PLAIN), (2, HISTORY), (2, HISTORY)),
    (True, False, True):          ((0, PLAIN), (0, PLAIN), (0, PLAIN),   (2, DICT)),
    (True, True, True):           ((0, PLAIN), (0, PLAIN), (0, PLAIN),   (2, DICT)),
}


def test_encode_route():
    assert len(HIGH) == 8
    for shape, routes in HIGH.items():
        for (hd, hl), want in zip(((0, 0), (1, 0), (0, 1), (1, 1)), routes):
            assert encode(2, hd, hl, *shape) == want, (shape, hd, hl)
            # modes 0 and 1 read neither setting and nothing of the call
            assert encode(0, hd, hl, *shape) == (0, PLAIN) and encode(1, hd, hl, *shape) == (1, PLAIN)


# ---------------------------------------------------------------------------------------------------------------- the lists
def listed(get, limit=64):
    out = []
    for i in range(limit):
        v = get(i)
        if v < 0:
            break
        out.append(v)
    return out


def test_tables_agree_with_the_library():
    from lz4_flex_amd import _lib
    m, lib = shim(), _lib.load()
    assert m.hr_chain_max_blocks() == 65536
    assert listed(m.hr_threshold) == THRESHOLDS and m.hr_threshold(-1) < 0
    assert listed(lambda i: lib.lz4flex_get_tuning(None, b"dispatch_threshold_%d" % i)) == THRESHOLDS
    assert listed(lambda i: m.hr_decoder_config(i, 0)) == CONFIGS and listed(lambda i: m.hr_decoder_config(i, 1)) == CONFIGS_TOOLS
    assert m.hr_decoder_config(-1, 0) < 0 and m.hr_decoder_config(-1, 1) < 0
    assert listed(lambda i: lib.lz4flex_get_tuning(None, b"decoder_config_%d" % i)) == CONFIGS          # (the product library is no tools build)
    for key in (b"decoder_config_", b"decoder_config_-1", b"decoder_config_x", b"dispatch_threshold_", b"dispatch_threshold_6", b"decoder_config_9"):
        assert lib.lz4flex_get_tuning(None, key) == -_lib.E_INVALID_ARG, key
    # every variant with a configuration is one the setting takes, and the other way round (0 has none: nothing is pinned)
    assert {c // 1000 for c in CONFIGS} == VARIANTS - {0} and {c // 1000 for c in CONFIGS_TOOLS} == VARIANTS_TOOLS - {0}
    for v in range(-2, 18):
        assert bool(m.hr_variant_ok(v, 0)) == (v in VARIANTS) and bool(m.hr_variant_ok(v, 1)) == (v in VARIANTS_TOOLS), v
    # the library's check: without a device every value is refused (no context), with one exactly the values outside the table
    have = lib.lz4flex_device_count() > 0
    before = lib.lz4flex_get_tuning(None, b"decompress_variant") if have else 0
    try:
        for v in range(-2, 18):
            rc = lib.lz4flex_set_tuning(None, b"decompress_variant", v)
            assert rc == ((0 if v in VARIANTS else -_lib.E_INVALID_ARG) if have else -_lib.E_NO_DEVICE), v
    finally:
        if have:
            assert lib.lz4flex_set_tuning(None, b"decompress_variant", before) == 0
