"""The frame layer's column sets (lz4_flex_amd/csrc/frame_cols.h) on the CPU: where every descriptor and result column of
frame_many.cpp, frame_index.cpp and sharded.cpp lies in its image, how much of the image lies in front of the upload boundary, and how
large the image is.  The device copy is scratch memory sized from these numbers and the kernels index it by them, so they are pinned.

The expected tables never come from the header: they are written here by hand from the byte counts the three files took, in their
order, before the columns had names (au = align up to 64): a column starts at the end so far, which then moves to au(end + bytes); a
column of no elements shares its start with its neighbour; up_bytes is the end behind the last column the host fills.  Each case names
the byte counts it was worked from."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sim", "frame_cols_shim.cpp")
HDRS = [os.path.join(ROOT, "lz4_flex_amd", "csrc", h) for h in ("frame_cols.h", "lz4_host_stage.h", "frame_range.h")]
SO = os.path.join(ROOT, "tests", "sim", "libframe_cols_shim.so")

ENCODE, HEADS, WALK, BATCH, SCRATCH, TABLE, PASS, SHARD_ENC, SHARD_DEC = range(9)
_m = None


def shim():
    global _m
    if _m is None:
        if not os.path.exists(SO) or max(os.path.getmtime(p) for p in [SRC] + HDRS) > os.path.getmtime(SO):
            subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-Wall", SRC, "-o", SO])
        m = C.CDLL(SO)
        m.fc_plan.restype = C.c_int
        m.fc_plan.argtypes = [C.c_uint32] + [C.POINTER(C.c_uint64)] * 3
        m.fc_view_offset.restype = C.c_uint64
        m.fc_view_offset.argtypes = [C.c_uint64]
        _m = m
    return _m


def plan(kind, counts):
    k = (C.c_uint64 * 4)(*(list(counts) + [0] * (4 - len(counts))))
    at, s = (C.c_uint64 * 32)(), (C.c_uint64 * 3)()
    n = shim().fc_plan(kind, k, at, s)
    assert n >= 0
    return {"cols": list(at[:n]), "up": s[0], "total": s[1], "tail": s[2]}


# (name, set, counts, column starts in declaration order, up_bytes, total)
CASES = [
    # frame_many.cpp encode (nf streams, nb blocks, Linked-exact): 56nf 8nf 4nf 8nb 8nb 4nb 4nb 4nb [40nb 4nf 4nf] | 4nb 4nb 8nb 8nb 4nb 4nb 4nf 8nf 4nf
    ("encode 3 streams 9 blocks chains", ENCODE, (3, 9, 1),
     [0, 192, 256, 320, 448, 576, 640, 704, 768, 1152, 1216, 1280, 1344, 1408, 1536, 1664, 1728, 1792, 1856, 1920], 1280, 1984),
    ("encode 3 streams 9 blocks", ENCODE, (3, 9, 0),      # cb / first / count of no elements: every later start as without them
     [0, 192, 256, 320, 448, 576, 640, 704, 768, 768, 768, 768, 832, 896, 1024, 1152, 1216, 1280, 1344, 1408], 768, 1472),
    ("encode 2 empty streams", ENCODE, (2, 0, 0),         # nb = 0
     [0, 128, 192] + [256] * 15 + [320, 384], 256, 448),
    ("encode 1 stream 1 block chains", ENCODE, (1, 1, 1), [64 * i for i in range(20)], 704, 1280),
    # decode H (n frames): 8n 8n | 32n
    ("heads 1", HEADS, (1,), [0, 64, 128], 128, 192),
    ("heads 3", HEADS, (3,), [0, 64, 128], 128, 256),
    # decode W (n frames, then `slots` table slots): 40n | 8slots 4slots 32n
    ("walk 3 frames 11 slots", WALK, (3, 11), [0, 128, 256, 320], 128, 448),
    ("walk 1 frame no slot", WALK, (1, 0), [0, 64, 64, 64], 64, 128),
    ("walk 5 frames 70 slots", WALK, (5, 70), [0, 256, 832, 1152], 256, 1344),
    # decode B (ne compressed, nr stored, nk checksums, n frames): 8ne 8ne 4ne 4ne 4ne 4ne 8nr 8nr 4nr 8nk 4nk | 4ne 4ne 16ne 4nk 4nk 8n 4n 4n
    ("batch 7 2 9 3", BATCH, (7, 2, 9, 3),
     [0, 64, 128, 192, 256, 320, 384, 448, 512, 576, 704, 768, 832, 896, 1024, 1088, 1152, 1216, 1280], 768, 1344),
    ("batch stored only", BATCH, (0, 3, 0, 1),            # nc = np = 0, nk = 0
     [0, 0, 0, 0, 0, 0, 0, 64, 128] + [192] * 8 + [256, 320], 192, 384),
    ("batch nothing stored", BATCH, (5, 0, 5, 2),         # nr = 0
     [0, 64, 128, 192, 256, 320, 384, 384, 384, 384, 448, 512, 576, 640, 768, 832, 896, 960, 1024], 512, 1088),
    ("batch no block at all", BATCH, (0, 0, 0, 1), [0] * 17 + [64, 128], 0, 192),
    # index_build scratch (mb blocks, mb / 1024 + 2 tiles), no host image: 8mb 4mb 16 4mb 8mb 4mb 8 8(mb + 1) 8tiles 64
    ("scratch 1 block", SCRATCH, (1, 2), [64 * i for i in range(10)], 0, 640),
    ("scratch 1030 blocks", SCRATCH, (1030, 3), [0, 8256, 12416, 12480, 16640, 24896, 29056, 29120, 37376, 37440], 0, 37504),
    ("scratch 2048 blocks", SCRATCH, (2048, 4), [0, 16384, 24576, 24640, 32832, 49216, 57408, 57472, 73920, 73984], 0, 74048),
    # the index's own copy (n blocks): 8(n + 1) 8n 4n
    ("table 0 blocks", TABLE, (0,), [0, 64, 64], 0, 64),
    ("table 3 blocks", TABLE, (3,), [0, 64, 128], 0, 192),
    ("table 9 blocks", TABLE, (9,), [0, 128, 256], 0, 320),
    # run_pass (R ranges, T slots): 64R | 8T 8T 4T 4T 4T 4T 8T 8T 4T 4T 4T 8R 8R 4R 4R 4R 4R 8R 8R 4R | 4R 4R 8R 8R 8R
    ("pass 3 ranges 5 slots", PASS, (3, 5), [0] + [192 + 64 * i for i in range(25)], 192, 1792),
    ("pass 1 range no slot", PASS, (1, 0), [0] + [64] * 12 + [128 + 64 * i for i in range(13)], 64, 960),      # T = 0
    ("pass 2 ranges 1 slot", PASS, (2, 1), [0] + [128 + 64 * i for i in range(25)], 128, 1728),
    # sharded encode (n blocks): 8n 8n 8n+8 4n 4n 4n 4n 4n | 16n
    ("shard encode 1", SHARD_ENC, (1,), [64 * i for i in range(9)], 512, 576),
    ("shard encode 5", SHARD_ENC, (5,), [64 * i for i in range(9)], 512, 640),
    # sharded decode (nc compressed, nr stored, n blocks): 8nc 8nc 8nr 8nr 8n 4nc 4nc 4nr 4n | 4nc 4nc 4n 4n
    ("shard decode 4 1 5", SHARD_DEC, (4, 1, 5), [64 * i for i in range(13)], 576, 832),
    ("shard decode stored only", SHARD_DEC, (0, 3, 3), [0, 0, 0, 64, 128, 192, 192, 192, 256, 320, 320, 320, 384], 320, 448),    # nc = 0
    ("shard decode nothing stored", SHARD_DEC, (3, 0, 3), [0, 64, 128, 128, 128, 192, 256, 320, 320, 384, 448, 512, 576], 384, 640),   # nr = 0
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_columns_match_the_hand_table(case):
    _, kind, counts, cols, up_bytes, total = case
    p = plan(kind, counts)
    assert p["cols"] == cols
    assert (p["up"], p["total"]) == (up_bytes, total)
    assert all(c % 64 == 0 for c in p["cols"]) and p["cols"] == sorted(p["cols"]) and p["up"] <= p["total"]


def test_every_set_has_two_shapes_and_its_empty_groups():
    kinds = [c[1] for c in CASES]
    assert all(kinds.count(k) >= 2 for k in range(9))
    counts = {k: [c[2] for c in CASES if c[1] == k] for k in range(9)}
    assert any(c[1] == 0 for c in counts[ENCODE]) and {c[2] for c in counts[ENCODE]} == {0, 1}          # nb = 0; Linked-exact absent and present
    assert any(c[0] == 0 for c in counts[BATCH]) and any(c[1] == 0 for c in counts[BATCH]) and any(c[2] == 0 for c in counts[BATCH])
    assert any(c[1] == 0 for c in counts[PASS]) and any(c[1] == 0 for c in counts[WALK])                # T = 0; no slot
    assert any(c[0] == 0 for c in counts[SHARD_DEC]) and any(c[1] == 0 for c in counts[SHARD_DEC]) and any(c[0] == 0 for c in counts[TABLE])


def test_the_verdict_columns_come_back_in_one_copy():
    # run_pass fetches from v_st to the end: 4R 4R 8R 8R 8R, each rounded up to 64
    assert [plan(PASS, c)["tail"] for c in ((3, 5), (1, 0), (2, 1), (9, 4))] == [320, 320, 320, 5 * 64 + 3 * 64]


def test_a_view_is_the_base_plus_the_columns_start():
    assert [shim().fc_view_offset(v) for v in (0, 64, 37440)] == [0, 64, 37440]


def test_an_unknown_set_is_refused():
    out = (C.c_uint64 * 32)()
    assert shim().fc_plan(9, out, out, out) == -1
