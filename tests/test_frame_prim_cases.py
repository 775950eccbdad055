"""CPU tests of tests/frame_prim_cases.py, the references and generators behind tests/test_gpu_frame_primitives.py: the numpy
assembler against sharded.build_segment's tensor-slice path, the Python walk against sharded.walk_blocks, the host lz4flex_xxh32
against the oracle on the grid the device kernel is tested on, and the generators against what they say they contain."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_prim_cases as F
import oracle_api as O


def oracle_xxh32_blocks(base, off, length, seed=0):
    raw = base.numpy().tobytes()
    return torch.tensor([O.xxh32(raw[int(o):int(o) + int(n)], seed) for o, n in zip(off.tolist(), length.tolist())], dtype=torch.int64)


@pytest.mark.parametrize("block_checksums", [False, True])
@pytest.mark.parametrize("n", [0, 1, 2, 1025])
def test_numpy_assembler_equals_build_segment(n, block_checksums):
    """on the layouts sharded.build_segment expresses (src_off = i * block_size), CPU tensors, the oracle's XXH32"""
    from lz4_flex_amd import sharded
    for variant in range(F.asm_variants(n)):
        c = F.asm_case(n, variant, F.ASM_BIG)
        assert (c["src_off"] == np.arange(n, dtype=np.uint64) * F.ASM_BIG).all()
        t = lambda k, dt: torch.from_numpy(np.array(c[k]).astype(dt))
        got = sharded.build_segment(t("src", np.uint8), t("comp", np.uint8), t("comp_off", np.int64), t("comp_len", np.int32), t("in_len", np.int32),
                                    F.ASM_BIG, block_checksums, oracle_xxh32_blocks)
        seg_off, seg = F.asm_reference(c, block_checksums)
        assert int(seg_off[n]) == len(seg) == got.numel()
        assert got.numpy().tobytes() == seg.tobytes()
        size = np.minimum(c["in_len"], c["comp_len"]).astype(np.uint64) + np.uint64(8 if block_checksums else 4)
        assert (np.diff(seg_off) == size).all() and (n == 0 or seg_off[0] == 0)


def test_python_walk_equals_walk_blocks():
    """on every valid frame of the walk's cases (sharded.walk_blocks has no max_blocks and raises where the frame does not parse)"""
    from lz4_flex_amd import frame, sharded
    seen = 0
    for c in F.walk_cases():
        k, st, end, offs, words = F.ref_walk(c["frame"], c["frame_len"], c["header_len"], c["block_checksums"], c["block_size"], c["max_blocks"])
        assert st == c["want"], c["name"]
        host = np.frombuffer(c["frame"], np.uint8)[:c["frame_len"]]
        if st == F.ST_OK:
            want, want_end = sharded.walk_blocks(host, c["header_len"], bool(c["block_checksums"]), c["block_size"])
            assert (k, end) == (len(want), want_end), c["name"]
            assert [(o, w & 0x7FFFFFFF, bool(w >> 31)) for o, w in zip(offs, words)] == want, c["name"]
            seen += 1
        elif st != F.ST_MAX_BLOCKS:
            with pytest.raises(frame.BlockTooBig if st == F.ST_TOO_BIG else ValueError):
                sharded.walk_blocks(host, c["header_len"], bool(c["block_checksums"]), c["block_size"])
    assert seen >= 6 * 8


def test_host_xxh32_equals_oracle_on_the_grid():
    """lz4flex_xxh32 (host, no device needed) on every length x phase x pattern x seed the device kernel is tested on"""
    from lz4_flex_amd import _lib, build
    build.build()
    lib = _lib.load()
    g = F.xxh_grid()
    at = g["base"].ctypes.data
    assert at % 16 == 0
    for seed in F.XXH_SEEDS:
        ref = F.xxh_reference(seed)
        got = np.array([lib.lz4flex_xxh32(C.c_void_p(at + int(o)), int(n), seed) for o, n in zip(g["off"], g["len"])], np.uint32)
        bad = np.nonzero(got != ref)[0]
        assert bad.size == 0, (hex(seed), int(g["len"][bad[0]]), int(g["phase"][bad[0]]))
    assert F.xxh_reference(0)[0] == 0x02CC5D05 and g["len"][0] == 0          # XXH32 of nothing, seed 0: the public test vector


def test_cases_contain_what_they_claim():
    g = F.xxh_grid()
    assert set(range(81)) | {255, 256, 257, 4095, 4096, 4097, 65536, 70001, (1 << 20) + 7} == set(g["len"].tolist())
    assert F.XXH_SEEDS == (0, 1, 0x9E3779B1, 0xFFFFFFFF) and F.XXH_SWEEP == (1, 3, 4, 15, 16, 17, 63, 64, 65, 127, 129, 1000)
    assert len(g["off"]) == len(F.XXH_LENGTHS) * 16 * 2
    assert ((g["off"] % 16) == g["phase"]).all()
    assert {(int(n), int(p), int(q)) for n, p, q in zip(g["len"], g["phase"], g["pattern"])} == {(n, p, q) for n in F.XXH_LENGTHS for p in range(16) for q in (0, 1)}
    ends = np.sort(g["off"]) [1:]
    order = np.argsort(g["off"])
    assert (g["off"][order][:-1] + g["len"][order][:-1] < ends).all()         # storage of their own, a byte between neighbours
    for o, n, q in zip(g["off"], g["len"], g["pattern"]):
        if q == 1:
            assert (g["base"][int(o):int(o) + int(n)] == 0xFF).all()
    assert sorted(g["len"][F.xxh_order("sorted")]) == g["len"][F.xxh_order("sorted")].tolist()
    sh = g["len"][F.xxh_order("shuffled")]
    assert sorted(F.xxh_order("shuffled").tolist()) == list(range(len(sh)))
    groups = sh[:len(sh) // 16 * 16].reshape(-1, 16)                           # the 16 buffers of a wavefront
    assert ((groups.max(axis=1) > (1 << 20)) & (groups.min(axis=1) == 0)).any()

    c = F.copy_case()
    triples = set(zip(c["sp"].tolist(), c["dp"].tolist(), c["len"].tolist()))
    assert len(triples) == len(c["len"])
    assert {(s, d, n) for s in range(16) for d in range(16) for n in F.COPY_LENGTHS} <= triples
    assert set(F.COPY_LENGTHS) == set(range(50)) | {255, 256, 257} | set(range(4080, 4113))
    for n in (8191, 8192, 8209, 70001):
        assert {(s, (s + 5) % 16, n) for s in range(16)} | {(s, s, n) for s in range(16)} <= triples
    assert ((c["src_off"] % 16) == c["sp"]).all() and ((c["dst_off"] % 16) == c["dp"]).all()
    order = np.argsort(c["dst_off"])
    lo, hi = c["dst_off"][order], c["dst_off"][order] + c["len"][order]
    assert lo[0] >= 16 and (lo[1:] >= hi[:-1] + np.uint64(16)).all() and c["dst_size"] == hi[-1] + F.TAIL
    assert (c["src_off"] + c["len"] <= len(c["pool"])).all()
    assert not (c["pool"] == F.CANARY).any() and int((c["image"] != F.CANARY).sum()) == int(c["len"].sum())

    assert F.ASM_NS == (0, 1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 3073)
    for n in F.ASM_NS:
        classes = set()
        for variant in range(F.asm_variants(n)):
            a = F.asm_case(n, variant)
            assert len(a["in_len"]) == n
            assert (a["comp_len"].astype(np.int64) == np.maximum(a["in_len"].astype(np.int64) + a["d"], 0)).all() and set(a["d"].tolist()) <= set(F.ASM_D)
            classes |= set(a["d"].tolist())
            if n >= 1023:
                assert set(a["d"].tolist()) == set(F.ASM_D)                   # every class in every batch
                assert {0, 1, F.ASM_BIG} <= set(a["in_len"].tolist()) and a["in_len"].max() == F.ASM_BIG
                assert len(set((a["src_off"] % 16).tolist())) == 16 and len(set((a["comp_off"] % 16).tolist())) == 16
                order = np.argsort(a["src_off"], kind="stable")
                assert (np.diff(a["src_off"][order].astype(np.int64)) >= a["in_len"][order][:-1]).all()
                assert (np.diff(a["src_off"][order].astype(np.int64)) > a["in_len"][order][:-1]).any()
            assert n == 0 or int((a["src_off"] + a["in_len"]).max()) <= len(a["src"])
            assert n == 0 or int((a["comp_off"] + a["comp_len"]).max()) <= len(a["comp"])
        assert n == 0 or classes == set(F.ASM_D)                              # (fewer than 5 blocks: over the five variants of the batch)

    cases = F.walk_cases()
    assert {c["group"] for c in cases} == set(F.WALK_GROUPS)
    assert {c["want"] for c in cases} == {F.ST_OK, F.ST_TRUNCATED, F.ST_TOO_BIG, F.ST_MAX_BLOCKS}
    assert {c["header_len"] for c in cases} == {0, 7, 19} and {c["block_checksums"] for c in cases} == {0, 1}
    want = {"valid": {F.ST_OK}, "too_big": {F.ST_TOO_BIG}, "cut": {F.ST_TRUNCATED}, "no_endmark": {F.ST_TRUNCATED}, "short": {F.ST_TRUNCATED},
            "max_blocks": {F.ST_MAX_BLOCKS, F.ST_OK}}
    counts = set()
    for c in cases:
        assert c["want"] in want[c["group"]] and c["frame_len"] <= len(c["frame"]), c["name"]
        k, st, end, offs, words = F.ref_walk(c["frame"], c["frame_len"], c["header_len"], c["block_checksums"], c["block_size"], c["max_blocks"])
        assert (k, st) == (c["blocks"], c["want"]), c["name"]
        if c["group"] == "valid":
            counts.add(k)
            assert k <= c["max_blocks"]
        if st == F.ST_MAX_BLOCKS:
            assert k == c["max_blocks"] < 5
        if c["name"].startswith("blocks of exactly"):
            assert [w & 0x7FFFFFFF for w in words].count(c["block_size"]) == 2 and {w >> 31 for w in words} == {0, 1}
        if "behind the EndMark" in c["name"]:
            assert end < c["frame_len"]
        if c["name"].startswith("inside the third payload"):
            assert k == 2 and offs[1] + (words[1] & 0x7FFFFFFF) + 4 * c["block_checksums"] + 4 < c["frame_len"]
    assert {0, 1, 5, 300} <= counts
    assert any(w == 0x80000000 for c in cases if c["group"] == "valid" for w in F.ref_walk(c["frame"], c["frame_len"], c["header_len"], c["block_checksums"],
                                                                                            c["block_size"], c["max_blocks"])[4])
    cuts = sorted(len(c["frame"]) - c["frame_len"] for c in cases if c["group"] == "cut" and c["header_len"] == 7 and c["block_checksums"] == 1 and "short" in c["name"])
    assert cuts == list(range(1, 17))
