"""The plan layer of lz4_flex_amd/csrc/lz4_host_stage.h on the CPU: where the descriptor / result columns of a MEM_HOST call lie in the
page-locked image, how much of it goes up, and where the regions lie in the arena.

Every offset decides which path a kernel takes (aligned or narrow) and whether its reads behind a region's last byte stay inside the
allocation, so the numbers are pinned.  The expected tables never come from the header: they are written here by hand from the rules
the host C ABI staged by before the helper existed (au = align up):
  columns    one behind the other, each start at the image's alignment (16; the small path: 64); take(bytes) returns the end so far and
             moves it to au(end + bytes, align); a column of 0 elements shares its start with its neighbour;
  up_bytes   the end behind the last `up` column;
  regions    the first at 0, each next one au(bytes + slack, 256) further; the data regions take slack 64; the column image is a region
             of total bytes, slack 0 (slack 64 in lz4flex_compress_chains); a work area behind it has slack 0;
  arena      the last region's start + its bytes + 256.
Each case lists the declarations a path of capi.cpp makes, in its order, and what they must yield."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sim", "host_stage_shim.cpp")
HDR = os.path.join(ROOT, "lz4_flex_amd", "csrc", "lz4_host_stage.h")
SO = os.path.join(ROOT, "tests", "sim", "libhost_stage_shim.so")

_m = None


def shim():
    global _m
    if _m is None:
        if not os.path.exists(SO) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(SO):
            subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-Wall", SRC, "-o", SO])
        m = C.CDLL(SO)
        m.hs_plan.restype = C.c_int
        m.hs_plan.argtypes = [C.c_uint64, C.POINTER(C.c_uint64), C.c_uint32] + [C.POINTER(C.c_uint64)] * 3
        _m = m
    return _m


def up(size, count):
    return (0, size, count)


def down(size, count):
    return (1, size, count)


def region(nbytes, slack):
    return (2, nbytes, slack)


def columns(slack=0):
    return (3, slack, 0)


def plan(align, ops):
    flat = (C.c_uint64 * (3 * len(ops)))(*[v for op in ops for v in op])
    at = (C.c_uint64 * len(ops))()
    room = (C.c_uint64 * len(ops))()
    s = (C.c_uint64 * 5)()
    assert shim().hs_plan(align, flat, len(ops), at, room, s) == 0
    return {"cols": [at[i] for i, op in enumerate(ops) if op[0] < 2], "regions": [at[i] for i, op in enumerate(ops) if op[0] >= 2],
            "rooms": [room[i] for i, op in enumerate(ops) if op[0] >= 2], "up": s[0], "total": s[1], "arena": s[2], "desc": s[3], "down": s[4]}


# (name, alignment, declarations, column starts, up_bytes, total, region starts (the column image among them), arena bytes)
CASES = [
    # 1 run_host_small: Layout{64}; in_off out_off in_len out_cap flags + the input slots | out_len status detail + the output slots; the
    #   image is the arena's one region.  A slot is au(len + 16, 64).
    #   n = 1, in_len 100 -> slot 128, out_cap 131 -> slot 192
    ("small n=1", 64,
     [up(8, 1), up(8, 1), up(4, 1), up(4, 1), up(4, 1), up(1, 128), down(4, 1), down(4, 1), down(8, 2), down(1, 192), columns()],
     [0, 64, 128, 192, 256, 320, 448, 512, 576, 640], 448, 832, [0], 1088),
    #   n = 5, in_len 0 1 48 49 700 -> slots 64 64 64 128 768 = 1088; out_cap 0 7 100 700 33 -> slots 64 64 128 768 64 = 1088
    ("small n=5", 64,
     [up(8, 5), up(8, 5), up(4, 5), up(4, 5), up(4, 5), up(1, 1088), down(4, 5), down(4, 5), down(8, 10), down(1, 1088), columns()],
     [0, 64, 128, 192, 256, 320, 1408, 1472, 1536, 1664], 1408, 2752, [0], 3008),
    # 2 run_host_batch: in_off out_off dict_off? in_len out_cap flags? dict_len? out_pos? dict_id? | out_len status detail; regions in, out,
    #   dict with 64 bytes of slack each, then the columns
    #   n = 9, every optional column; 5000 / 9001 / 300 bytes
    ("batch n=9 all", 16,
     [up(8, 9), up(8, 9), up(8, 9), up(4, 9), up(4, 9), up(4, 9), up(4, 9), up(4, 9), up(4, 9), down(4, 9), down(4, 9), down(8, 18),
      region(5000, 64), region(9001, 64), region(300, 64), columns()],
     [0, 80, 160, 240, 288, 336, 384, 432, 480, 528, 576, 624], 528, 768, [0, 5120, 14336, 14848], 15872),
    #   n = 9, none of them: four columns of 0 elements share their start with their neighbour; the empty dictionary region still has room
    ("batch n=9 none", 16,
     [up(8, 9), up(8, 9), up(8, 0), up(4, 9), up(4, 9), up(4, 0), up(4, 0), up(4, 0), up(4, 0), down(4, 9), down(4, 9), down(8, 18),
      region(5000, 64), region(9001, 64), region(0, 64), columns()],
     [0, 80, 160, 160, 208, 256, 256, 256, 256, 256, 304, 352], 256, 496, [0, 5120, 14336, 14592], 15344),
    #   n = 5 with flags; 1 byte in, 192 out: 192 + 64 is a multiple of 256 already
    ("batch n=5 flags", 16,
     [up(8, 5), up(8, 5), up(8, 0), up(4, 5), up(4, 5), up(4, 5), up(4, 0), up(4, 0), up(4, 0), down(4, 5), down(4, 5), down(8, 10),
      region(1, 64), region(192, 64), region(0, 64), columns()],
     [0, 48, 96, 96, 128, 160, 192, 192, 192, 192, 224, 256], 192, 336, [0, 256, 512, 768], 1360),
    # 3 lz4flex_decompressed_size_batch: in_off in_len history? | out_size status; region in, then the columns
    ("size n=1", 16, [up(8, 1), up(4, 1), up(4, 0), down(8, 1), down(4, 1), region(0, 64), columns()],
     [0, 16, 32, 32, 48], 32, 64, [0, 256], 576),
    ("size n=5 history", 16, [up(8, 5), up(4, 5), up(4, 5), down(8, 5), down(4, 5), region(193, 64), columns()],
     [0, 48, 80, 112, 160], 112, 192, [0, 512], 960),
    # 4 lz4flex_decompress_batch_packed: in_off in_len sizes? | out_off (8 n + 8) out_cap out_len status detail; region in, the columns
    #   rounded WITHOUT slack, the work area
    ("packed decode n=9 given", 16,
     [up(8, 9), up(4, 9), up(4, 9), down(8, 10), down(4, 9), down(4, 9), down(4, 9), down(8, 18), region(4099, 64), columns(), region(1000, 0)],
     [0, 80, 128, 176, 256, 304, 352, 400], 176, 544, [0, 4352, 5120], 6376),
    ("packed decode n=1", 16,
     [up(8, 1), up(4, 1), up(4, 0), down(8, 2), down(4, 1), down(4, 1), down(4, 1), down(8, 2), region(5, 64), columns(), region(77, 0)],
     [0, 16, 32, 32, 48, 64, 80, 96], 32, 112, [0, 256, 512], 845),
    # 5 lz4flex_compress_batch_packed: in_off in_len | out_off (8 n + 8) out_len status
    ("packed compress n=5", 16, [up(8, 5), up(4, 5), down(8, 6), down(4, 5), down(4, 5), region(2000, 64), columns(), region(640, 0)],
     [0, 48, 80, 128, 160], 80, 192, [0, 2304, 2560], 3456),
    ("packed compress n=9", 16, [up(8, 9), up(4, 9), down(8, 10), down(4, 9), down(4, 9), region(70000, 64), columns(), region(1000, 0)],
     [0, 80, 128, 208, 256], 128, 304, [0, 70144, 70656], 71912),
    # 6 lz4flex_dict_train: in_off in_len | two result words, dict_cap bytes
    ("train n=1", 16, [up(8, 1), up(4, 1), down(4, 2), down(1, 100), region(700, 64), columns(), region(500, 0)],
     [0, 16, 32, 48], 32, 160, [0, 768, 1024], 1780),
    ("train n=5 64K", 16, [up(8, 5), up(4, 5), down(4, 2), down(1, 65536), region(3000, 64), columns(), region(4096, 0)],
     [0, 48, 80, 96], 80, 65632, [0, 3072, 68864], 73216),
    # 7 typed_on_host: in_off out_off tmp_off in_len out_cap | out_len status detail; regions in, tmp, out, then the columns
    ("typed compress n=5", 16,
     [up(8, 5), up(8, 5), up(8, 5), up(4, 5), up(4, 5), down(4, 5), down(4, 5), down(8, 10), region(1500, 64), region(1500, 64), region(2100, 64),
      columns()],
     [0, 48, 96, 144, 176, 208, 240, 272], 208, 352, [0, 1792, 3584, 5888], 6496),
    ("typed filter n=9", 16,
     [up(8, 9), up(8, 9), up(8, 9), up(4, 9), up(4, 9), down(4, 9), down(4, 9), down(8, 18), region(900, 64), region(0, 64), region(900, 64),
      columns()],
     [0, 80, 160, 240, 288, 336, 384, 432], 336, 576, [0, 1024, 1280, 2304], 3136),
    # 8 fit_on_host: blk_off src_off out_off blk_len src_len out_cap | out_len in_used status; regions blk, src, out, the columns without
    #   slack, the work area (compress; else 0 bytes)
    ("fit n=1", 16,
     [up(8, 1), up(8, 1), up(8, 1), up(4, 1), up(4, 1), up(4, 1), down(4, 1), down(4, 1), down(4, 1), region(50, 64), region(120, 64),
      region(30, 64), columns(), region(0, 0)],
     [0, 16, 32, 48, 64, 80, 96, 112, 128], 96, 144, [0, 256, 512, 768, 1024], 1280),
    ("fit compress n=9", 16,
     [up(8, 9), up(8, 9), up(8, 9), up(4, 9), up(4, 9), up(4, 9), down(4, 9), down(4, 9), down(4, 9), region(0, 64), region(6000, 64),
      region(3000, 64), columns(), region(1000, 0)],
     [0, 80, 160, 240, 288, 336, 384, 432, 480], 384, 528, [0, 256, 6400, 9472, 10240], 11496),
    # lz4flex_compress_chains: blocks (40 bytes each) first count out_off out_cap | out_len status; regions in, out, the columns WITH 64
    #   bytes of slack, the table state
    ("chains 5 blocks 2 chains", 16,
     [up(40, 5), up(4, 2), up(4, 2), up(8, 5), up(4, 5), down(4, 5), down(4, 5), region(1000, 64), region(2000, 64), columns(64), region(32768, 0)],
     [0, 208, 224, 240, 288, 320, 352], 320, 384, [0, 1280, 3584, 4096], 37120),
    ("chains 1 block", 16,
     [up(40, 1), up(4, 1), up(4, 1), up(8, 1), up(4, 1), down(4, 1), down(4, 1), region(10, 64), region(20, 64), columns(64), region(0, 0)],
     [0, 48, 64, 80, 96, 112, 128], 112, 144, [0, 256, 512, 768], 1024),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_plan_matches_the_hand_table(case):
    _, align, ops, cols, up_bytes, total, regions, arena = case
    p = plan(align, ops)
    assert p["cols"] == cols
    assert (p["up"], p["total"]) == (up_bytes, total)
    assert p["regions"] == regions
    assert p["arena"] == arena
    # the column image is the region declared by columns(); "from the first down column to the end" is what comes back
    assert p["desc"] == regions[[op[0] for op in ops if op[0] >= 2].index(3)]
    assert p["down"] == total - up_bytes
    # every column starts at the alignment and every region at a multiple of 256, with room for its bytes and its slack
    assert all(c % align == 0 for c in p["cols"]) and all(r % 256 == 0 for r in p["regions"])
    for (kind, a, b), room in zip([op for op in ops if op[0] >= 2], p["rooms"]):
        nbytes, slack = (a, b) if kind == 2 else (total, a)
        assert room % 256 == 0 and nbytes + slack <= room < nbytes + slack + 256


def test_every_path_has_two_shapes():
    names = [c[0].split(" ")[0] for c in CASES]
    # ("packed" and "fit" are two entry points each)
    assert {n: names.count(n) for n in set(names)} == {"small": 2, "batch": 3, "size": 2, "packed": 4, "train": 2, "typed": 2, "fit": 2, "chains": 2}


def test_a_column_of_no_elements_shares_its_start():
    p = plan(16, [up(8, 3), up(4, 0), up(8, 0), up(4, 3), down(4, 0), down(8, 3), region(10, 64), columns()])
    assert p["cols"] == [0, 32, 32, 32, 48, 48]
    assert (p["up"], p["total"], p["down"]) == (48, 80, 32)
    # ... and an empty plan is an empty image in an arena of the closing 256 bytes
    q = plan(16, [columns()])
    assert (q["up"], q["total"], q["regions"], q["arena"]) == (0, 0, [0], 256)


def test_an_unknown_declaration_is_refused():
    flat = (C.c_uint64 * 3)(7, 0, 0)
    out = (C.c_uint64 * 5)()
    assert shim().hs_plan(16, flat, 1, out, out, out) == -1
    flat = (C.c_uint64 * 3)(0, 3, 1)      # an element size the shim has no type for
    assert shim().hs_plan(16, flat, 1, out, out, out) == -1
