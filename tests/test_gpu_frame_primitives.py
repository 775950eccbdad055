"""The frame layer's four device entry points (include/lz4flex_amd.h: lz4flex_xxh32_batch_device, lz4flex_copy_batch_device,
lz4flex_frame_assemble_device, lz4flex_frame_walk_device) called through the C ABI with device tensors and compared, exactly and
whole, with the plain references of tests/frame_prim_cases.py: every array the library writes starts as canary and must come back as
the expected values plus canary, so a write outside a range fails like a wrong byte inside one.  tests/test_frame_prim_cases.py pins
the references themselves."""
import numpy as np
import pytest

import frame_prim_cases as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from lz4_flex_amd import _lib
    L = _lib.load()
    assert L.lz4flex_device_count() >= 1
    return L


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d entries differ from the reference / the canary, first at %d: got %#x, want %#x" % (
        what, bad.size, bad[0], int(got[bad[0]]), int(want[bad[0]]))


# ---- 1. XXH32 -------------------------------------------------------------------------------------------------------------------
class TestXxh32:
    @pytest.fixture(scope="class")
    def d_base(self, lib):
        import torch
        t = F._dev(F.xxh_grid()["base"])
        yield t
        del t
        torch.cuda.empty_cache()

    @pytest.mark.parametrize("order", ["sorted", "shuffled"])
    @pytest.mark.parametrize("seed", F.XXH_SEEDS)
    def test_every_length_phase_and_pattern(self, lib, d_base, seed, order):
        """lengths 0..80 (every length mod 16 with 0 to 5 stripes), around 256 and 4 096, 64 KiB, 70 001 and 1 MiB + 7, each at the 16
        phases of base + off, random bytes and all 0xFF, one launch: == the oracle's XXH32 with this seed.  Shuffled, a group of a
        wavefront leaves the stripe loop 65 536 iterations before its neighbour."""
        g = F.xxh_grid()
        idx = F.xxh_order(order)
        rc, out = F.xxh32_device(lib, d_base, g["off"][idx], g["len"][idx], seed)
        assert rc == 0
        same(out, F.xxh_image(F.xxh_reference(seed)[idx]), "seed %#x, %s" % (seed, order))

    @pytest.mark.parametrize("n", F.XXH_SWEEP)
    def test_batch_sizes_around_group_wavefront_and_workgroup(self, lib, d_base, n):
        """4 lanes a buffer, 16 buffers a wavefront, 64 a workgroup: batches that end inside each of them, mixed lengths; out[n] survives"""
        g = F.xxh_grid()
        idx = np.roll(F.xxh_order("shuffled"), -7 * n)[:n]
        assert n < 4 or len(set(g["len"][idx].tolist())) > 1
        rc, out = F.xxh32_device(lib, d_base, g["off"][idx], g["len"][idx], 1)
        assert rc == 0
        same(out, F.xxh_image(F.xxh_reference(1)[idx]), "n = %d" % n)

    def test_empty_batch_writes_nothing(self, lib, d_base):
        rc, out = F.xxh32_device(lib, d_base, np.zeros(0, np.uint64), np.zeros(0, np.uint32), 0)
        assert rc == 0
        same(out, F.xxh_image([]), "n = 0")


# ---- 2. copy batch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["as laid out", "shuffled"])
def test_copy_batch_every_phase_pair(lib, order):
    """every (source phase, destination phase) pair x lengths 0..49, 255..257 and 4 080..4 112 (one pass of 256 lanes x 16 B around its
    end, the head taken off by the destination's phase), 8 191 .. 70 001 at the pairs (s, s) and (s, s + 5): one launch; the destination
    == numpy's slices, canary between the ranges (16 bytes at least) and behind the last.  The same ranges in another order of the batch:
    the same destination."""
    c = F.copy_case()
    n = len(c["len"])
    idx = np.arange(n) if order == "as laid out" else np.random.default_rng(0x5EED06).permutation(n)
    rc, dst = F.copy_device(lib, F._dev(c["pool"]), c["src_off"][idx], c["len"][idx], c["dst_off"][idx], c["dst_size"])
    assert rc == 0
    same(dst, c["image"], "copy batch, %s" % order)


def test_copy_batch_empty(lib):
    c = F.copy_case()
    rc, dst = F.copy_device(lib, F._dev(c["pool"]), np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint64), F.TAIL)
    assert rc == 0
    same(dst, np.full(F.TAIL, F.CANARY, np.uint8), "n = 0")


# ---- 3. frame assembly -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block_checksums", [False, True])
@pytest.mark.parametrize("n", F.ASM_NS)
def test_frame_assemble(lib, n, block_checksums):
    """n blocks (1 to 4 per thread of the size scan, ragged last threads, threads with nothing to do) whose compressed length lies 2 and 1
    below, at, and 1 and 5 above the input's, sources and payloads at arbitrary byte phases: all n + 1 offsets, the segment and the
    canaries behind both == the rule restated in numpy, checksums from the oracle; seg has exactly sum(in_len) + 8 n bytes"""
    for variant in range(F.asm_variants(n)):
        c = F.asm_case(n, variant)
        rc, seg_off, seg, behind_scratch = F.asm_device(lib, c, block_checksums)
        assert rc == 0
        want_off, want_seg = F.asm_images(c, block_checksums)
        what = "n = %d, variant %d, checksums %d" % (n, variant, block_checksums)
        same(seg_off, want_off, what + ": seg_off")
        same(seg, want_seg, what + ": seg")
        if block_checksums:
            same(behind_scratch, np.full(F.TAIL, F.CANARY, np.uint8), what + ": behind scratch")


# ---- 4. frame walk ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", F.WALK_GROUPS)
def test_frame_walk(lib, group):
    """hand-written frames == the Python walk: info[0] and info[1] always, info[2..3] with status 0, the tables' entries and the canary in
    every slot from info[0] on (a block that is refused leaves no entry)"""
    cases = [c for c in F.walk_cases() if c["group"] == group]
    assert cases
    for c in cases:
        slots = c["max_blocks"] + F.PAD
        rc, info, off, word = F.walk_device(lib, c, slots)
        assert rc == 0, c["name"]
        st, want_info, want_off, want_word = F.walk_images(c, slots)
        assert st == c["want"], c["name"]
        for i, w in enumerate(want_info):
            assert w is None or int(info[i]) == w, "%s: info[%d] = %#x, want %#x (info %s)" % (c["name"], i, int(info[i]), w, info[:4])
        same(off, want_off, c["name"] + ": payload_off")
        same(word, want_word, c["name"] + ": len_word")
