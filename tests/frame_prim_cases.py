"""What tests/test_gpu_frame_primitives.py and tests/test_frame_prim_cases.py share: the cases, the plain references and the C-ABI calls
for the four device entry points of the frame layer (include/lz4flex_amd.h: lz4flex_xxh32_batch_device, lz4flex_copy_batch_device,
lz4flex_frame_assemble_device, lz4flex_frame_walk_device).  Every generator is deterministic (fixed seeds, cached: one copy per
process, never modified), every call helper fills each array the library writes with canaries first and returns it WHOLE, so a test
compares it against an image of expected values plus canary.  A plain module, not a fixture."""
import ctypes as C
import functools

import numpy as np

import oracle_api as O

CANARY = 0xC5
CANARY32 = 0xC5C5C5C5
CANARY64 = 0xC5C5C5C5C5C5C5C5
TAIL = 512                      # canary bytes behind a byte buffer
PAD = 16                        # canary entries behind a result array
UNCOMPRESSED_BIT = 0x80000000


def _no_canary(a):
    """payload bytes never equal the canary, so a byte that was not written is always seen"""
    a[a == CANARY] = 0x3A
    return a


def _aligned(n, align=64):
    """n writable bytes whose address is a multiple of `align` (the phases below are those of base + off)"""
    raw = np.zeros(n + align, np.uint8)
    skip = (-raw.ctypes.data) % align
    out = raw[skip:skip + n]
    assert out.ctypes.data % align == 0
    return out


def _dev(a):
    import torch
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    t = torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))
    assert t.data_ptr() % 16 == 0
    return t


def _host(t, dt):
    return t.cpu().numpy().view(dt)


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else None)


def _stream(t):
    import torch
    return torch.cuda.current_stream(t.device)


# ---- 1. XXH32 -------------------------------------------------------------------------------------------------------------------
XXH_LENGTHS = tuple(range(81)) + (255, 256, 257, 4095, 4096, 4097, 65536, 70001, (1 << 20) + 7)
XXH_SEEDS = (0, 1, 0x9E3779B1, 0xFFFFFFFF)
XXH_PATTERNS = ("random", "ff")
XXH_SWEEP = (1, 3, 4, 15, 16, 17, 63, 64, 65, 127, 129, 1000)


@functools.lru_cache(maxsize=None)
def xxh_grid():
    """every length x phase 0..15 x pattern, each buffer with storage of its own and at least one foreign byte on both sides:
    dict(base: uint8 at a 64-aligned address, off u64, len u32, phase, pattern: index into XXH_PATTERNS), sorted by length"""
    offs, lens, phases, pats, at = [], [], [], [], 1
    for ln in XXH_LENGTHS:
        for pat in range(len(XXH_PATTERNS)):
            for ph in range(16):
                at += 1 + (ph - (at + 1)) % 16
                offs.append(at); lens.append(ln); phases.append(ph); pats.append(pat)
                at += ln
    base = _aligned(at + 64)
    base[:] = np.random.default_rng(0x5EED01).integers(0, 256, base.size, dtype=np.uint8)
    for o, ln, pat in zip(offs, lens, pats):
        if XXH_PATTERNS[pat] == "ff":
            base[o:o + ln] = 0xFF
    g = dict(base=base, off=np.array(offs, np.uint64), len=np.array(lens, np.uint32), phase=np.array(phases), pattern=np.array(pats))
    for v in g.values():
        v.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def xxh_reference(seed):
    """the oracle's XXH32 of every buffer of the grid, u32"""
    g = xxh_grid()
    ref = np.array([O.xxh32(g["base"][int(o):int(o) + int(n)].tobytes(), seed) for o, n in zip(g["off"], g["len"])], np.uint32)
    ref.setflags(write=False)
    return ref


def xxh_order(kind):
    """indices into the grid: "sorted" by length, or "shuffled" with a fixed seed (a 1 MiB buffer next to an empty one)"""
    n = len(xxh_grid()["off"])
    if kind == "sorted":
        return np.arange(n)
    assert kind == "shuffled"
    return np.random.default_rng(0x5EED02).permutation(n)


def xxh32_device(lib, d_base, off, length, seed):
    """lz4flex_xxh32_batch_device over a base that is on the device already; returns out[0 .. n + PAD), canary before the call"""
    n = len(off)
    d_out = _dev(np.full(n + PAD, CANARY32, np.uint32))
    d_off, d_len = _dev(np.ascontiguousarray(off, np.uint64)), _dev(np.ascontiguousarray(length, np.uint32))
    s = _stream(d_base)
    rc = lib.lz4flex_xxh32_batch_device(_p(d_base), _p(d_off), _p(d_len), n, int(seed), _p(d_out), C.c_void_p(s.cuda_stream))
    s.synchronize()
    return rc, _host(d_out, np.uint32)


def xxh_image(ref):
    return np.concatenate([np.asarray(ref, np.uint32), np.full(PAD, CANARY32, np.uint32)])


# ---- 2. copy batch ---------------------------------------------------------------------------------------------------------------
COPY_LENGTHS = tuple(range(50)) + (255, 256, 257) + tuple(range(4080, 4113))
COPY_EXTRA = (8191, 8192, 8209, 70001)
COPY_POOL = 1 << 20
COPY_GAP = 16


@functools.lru_cache(maxsize=None)
def copy_case():
    """dict(pool: the source bytes; src_off, len, dst_off; sp, dp: the two phases of every range; dst_size; image: the destination
    as it must look afterwards, canary wherever no range lies).  Source ranges overlap one another in a 1 MiB pool (they are only
    read); destination ranges are at least COPY_GAP canary bytes apart and TAIL canary bytes follow the last."""
    rng = np.random.default_rng(0x5EED03)
    pool = _no_canary(rng.integers(0, 256, COPY_POOL, dtype=np.uint8))
    todo = [(sp, dp, ln) for sp in range(16) for dp in range(16) for ln in COPY_LENGTHS]
    todo += [(s, (s + 5) % 16, ln) for s in range(16) for ln in COPY_EXTRA] + [(s, s, ln) for s in range(16) for ln in COPY_EXTRA]
    todo = [todo[i] for i in rng.permutation(len(todo))]                # neighbours in the destination are of mixed kinds
    src_off, dst_off, at = [], [], 0
    for sp, dp, ln in todo:
        r = int(rng.integers(0, (COPY_POOL - ln - 32) // 16))
        src_off.append(16 * r + sp)
        at += COPY_GAP
        at += (dp - at) % 16
        dst_off.append(at)
        at += ln
    dst_size = at + TAIL
    image = np.full(dst_size, CANARY, np.uint8)
    for s, d, (_, _, ln) in zip(src_off, dst_off, todo):
        image[d:d + ln] = pool[s:s + ln]
    c = dict(pool=pool, src_off=np.array(src_off, np.uint64), len=np.array([t[2] for t in todo], np.uint32), dst_off=np.array(dst_off, np.uint64),
             sp=np.array([t[0] for t in todo]), dp=np.array([t[1] for t in todo]), image=image)
    for v in c.values():
        v.setflags(write=False)
    c["dst_size"] = dst_size
    return c


def copy_device(lib, d_src, src_off, length, dst_off, dst_size):
    """lz4flex_copy_batch_device into a destination of dst_size canary bytes; returns the destination whole"""
    n = len(src_off)
    d_dst = _dev(np.full(dst_size, CANARY, np.uint8))
    d_so, d_ln, d_do = _dev(np.ascontiguousarray(src_off, np.uint64)), _dev(np.ascontiguousarray(length, np.uint32)), _dev(np.ascontiguousarray(dst_off, np.uint64))
    s = _stream(d_src)
    rc = lib.lz4flex_copy_batch_device(_p(d_src), _p(d_so), _p(d_ln), _p(d_dst), _p(d_do), n, C.c_void_p(s.cuda_stream))
    s.synchronize()
    return rc, _host(d_dst, np.uint8)


# ---- 3. frame assembly -----------------------------------------------------------------------------------------------------------
ASM_NS = (0, 1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 3073)
ASM_D = (-2, -1, 0, 1, 5)                # comp_len - in_len: the store-raw boundary (comp_len >= in_len) from both sides
ASM_BIG = 5000


def asm_variants(n):
    """a batch of fewer than 5 blocks cannot hold the five classes of ASM_D: it is built five times, the classes rotated through its blocks"""
    return 5 if 0 < n < len(ASM_D) else 1


@functools.lru_cache(maxsize=None)
def asm_case(n, variant=0, block_size=None):
    """n blocks: dict(src, src_off, in_len, comp, comp_off, comp_len, d).  in_len from 0..300 with a few blocks of ASM_BIG and a few of 0 and
    1; comp_len = max(in_len + d, 0), block i of class ASM_D[(i + variant) % 5] in a shuffled numbering, and a block of a negative class
    is long enough not to be clipped; both payloads at arbitrary byte phases with gaps of 0..37 bytes, random bytes.  block_size: the layout
    sharded.build_segment expresses instead (src_off = i * block_size)."""
    rng = np.random.default_rng([0x5EED04, n, variant])
    in_len = rng.integers(0, 301, n).astype(np.int64)
    if n >= 16:
        special = rng.permutation(n)[:12]
        in_len[special[:4]] = ASM_BIG
        in_len[special[4:8]] = 0
        in_len[special[8:]] = 1
    elif n:
        in_len[:] = np.array([37, 300, ASM_BIG, 2, 16])[(np.arange(n) + 2 * variant) % 5]
    cls = (rng.permutation(n) + variant) % len(ASM_D)
    d = np.array(ASM_D)[cls] if n else np.zeros(0, np.int64)
    in_len = np.where((d < 0) & (in_len < 2), in_len + 2, in_len)
    comp_len = np.maximum(in_len + d, 0)
    if block_size is None:
        src_off = np.cumsum(in_len + rng.integers(0, 38, n)) - in_len + 3 if n else np.zeros(0, np.int64)
        src_size = int((src_off + in_len).max()) + 8 if n else 8
    else:
        assert n == 0 or in_len.max() <= block_size
        src_off = np.arange(n, dtype=np.int64) * block_size
        src_size = max(n * block_size, 8)
    comp_off = np.cumsum(comp_len + rng.integers(0, 38, n)) - comp_len + 5 if n else np.zeros(0, np.int64)
    comp_size = int((comp_off + comp_len).max()) + 8 if n else 8
    c = dict(src=_no_canary(rng.integers(0, 256, src_size, dtype=np.uint8)), src_off=src_off.astype(np.uint64), in_len=in_len.astype(np.uint32),
             comp=_no_canary(rng.integers(0, 256, comp_size, dtype=np.uint8)), comp_off=comp_off.astype(np.uint64), comp_len=comp_len.astype(np.uint32),
             d=comp_len - in_len)
    for v in c.values():
        v.setflags(write=False)
    return c


def asm_reference(c, block_checksums, xxh32=O.xxh32):
    """The rule of lz4flex_frame_assemble_device's header comment restated: block i is stored raw iff comp_len >= in_len; its 4-byte header
    word is in_len | 0x80000000 or comp_len; the payload follows, then (block checksums) the XXH32 of the payload, seed 0, little endian; the
    blocks lie back to back.  Returns (seg_off: n + 1 u64, the last one the total; seg: the bytes)."""
    n = len(c["in_len"])
    seg_off = np.zeros(n + 1, np.uint64)
    seg = bytearray()
    for i in range(n):
        u, k = int(c["in_len"][i]), int(c["comp_len"][i])
        seg_off[i] = len(seg)
        if k >= u:
            word, at, base, size = u | UNCOMPRESSED_BIT, int(c["src_off"][i]), c["src"], u
        else:
            word, at, base, size = k, int(c["comp_off"][i]), c["comp"], k
        payload = base[at:at + size].tobytes()
        seg += word.to_bytes(4, "little") + payload
        if block_checksums:
            seg += xxh32(payload, 0).to_bytes(4, "little")
    seg_off[n] = len(seg)
    return seg_off, np.frombuffer(bytes(seg), np.uint8)


def asm_device(lib, c, block_checksums):
    """lz4flex_frame_assemble_device: seg has exactly the sum(in_len) + 8 n bytes the header asks for and TAIL canary bytes behind them,
    seg_off n + 1 entries and PAD canaries, scratch (NULL without block checksums) 16 n bytes and TAIL canary bytes.  Returns
    (rc, seg_off whole, seg whole, the bytes behind scratch or None)."""
    import torch
    n = len(c["in_len"])
    room = int(c["in_len"].sum(dtype=np.uint64)) + 8 * n
    d_src, d_comp = _dev(c["src"]), _dev(c["comp"])
    d = {k: _dev(np.array(c[k])) if n else None for k in ("src_off", "in_len", "comp_off", "comp_len")}
    d_seg = _dev(np.full(room + TAIL, CANARY, np.uint8))
    d_seg_off = _dev(np.full(n + 1 + PAD, CANARY64, np.uint64))
    d_scratch = _dev(np.full(16 * n + TAIL, CANARY, np.uint8)) if block_checksums else None
    s = _stream(d_src)
    rc = lib.lz4flex_frame_assemble_device(_p(d_src), _p(d["src_off"]), _p(d["in_len"]), _p(d_comp), _p(d["comp_off"]), _p(d["comp_len"]), n,
                                           1 if block_checksums else 0, _p(d_seg), _p(d_seg_off), _p(d_scratch), C.c_void_p(s.cuda_stream))
    s.synchronize()
    return rc, _host(d_seg_off, np.uint64), _host(d_seg, np.uint8), None if d_scratch is None else _host(d_scratch, np.uint8)[16 * n:]


def asm_images(c, block_checksums):
    """(seg_off, seg) as asm_device must return them"""
    n = len(c["in_len"])
    off, seg = asm_reference(c, block_checksums)
    room = int(c["in_len"].sum(dtype=np.uint64)) + 8 * n
    assert len(seg) <= room
    image = np.full(room + TAIL, CANARY, np.uint8)
    image[:len(seg)] = seg
    return np.concatenate([off, np.full(PAD, CANARY64, np.uint64)]), image


# ---- 4. frame walk ---------------------------------------------------------------------------------------------------------------
WALK_BLOCK_SIZE = 1000
ST_OK, ST_TRUNCATED, ST_TOO_BIG, ST_MAX_BLOCKS = 0, 1, 2, 3


def ref_walk(frame, frame_len, header_len, block_checksums, block_size, max_blocks):
    """FrameDecoder::read_block's walk over the BlockInfo words (src/frame/decompress.rs:231-247: four bytes little endian, 0 is the EndMark,
    the high bit says stored, a length above the block size is BlockTooBig before anything of the block is read) with the verdicts of
    lz4flex_frame_walk_device's header comment: 1 where the frame ends inside a word, a payload or a checksum, 3 where a complete block
    finds no table slot.  Returns (blocks, status, offset behind the EndMark or None, [payload_off], [len_word])."""
    tail = 4 if block_checksums else 0
    offs, words, p = [], [], header_len
    while True:
        if p + 4 > frame_len:
            return len(offs), ST_TRUNCATED, None, offs, words
        w = int.from_bytes(bytes(frame[p:p + 4]), "little")
        p += 4
        if w == 0:
            return len(offs), ST_OK, p, offs, words
        ln = w & ~UNCOMPRESSED_BIT
        if ln > block_size:
            return len(offs), ST_TOO_BIG, None, offs, words
        if p + ln + tail > frame_len:
            return len(offs), ST_TRUNCATED, None, offs, words
        if len(offs) >= max_blocks:
            return len(offs), ST_MAX_BLOCKS, None, offs, words
        offs.append(p); words.append(w)
        p += ln + tail


def make_frame(rng, header_len, blocks, block_checksums, endmark=True, behind=b""):
    """header_len bytes that are no header (the walk never reads them), then [word | payload | (4 bytes)] per (length, stored) of `blocks`,
    the EndMark, `behind`; (length, stored, present): a block of which only `present` bytes follow its word"""
    f = bytearray(rng.integers(1, 256, header_len, dtype=np.uint8).tobytes())
    for ln, stored, *present in blocks:
        f += (ln | (UNCOMPRESSED_BIT if stored else 0)).to_bytes(4, "little")
        f += rng.integers(1, 256, present[0] if present else ln + (4 if block_checksums else 0), dtype=np.uint8).tobytes()
    if endmark:
        f += bytes(4)
    return bytes(f + behind)


@functools.lru_cache(maxsize=None)
def walk_cases():
    """[dict(group, name, frame, frame_len, header_len, block_checksums, block_size, max_blocks, want: the status the case is there for,
    blocks: the count it must report)].
    `frame` may be longer than frame_len: a cut frame keeps its bytes behind the cut, so a walk that ignores frame_len ends with status 0."""
    rng = np.random.default_rng(0x5EED05)
    cases = []

    def add(group, name, frame, hl, bc, want, blocks, frame_len=None, block_size=WALK_BLOCK_SIZE, max_blocks=320):
        cases.append(dict(group=group, name="%s hl=%d bc=%d" % (name, hl, bc), frame=frame, frame_len=len(frame) if frame_len is None else frame_len,
                          header_len=hl, block_checksums=bc, block_size=block_size, max_blocks=max_blocks, want=want, blocks=blocks))

    def some(k, lo=1, hi=40):
        # k blocks of lo..hi bytes, among five a zero-length stored one (word 0x80000000: not the EndMark), a stored and a compressed one
        b = [(int(rng.integers(lo, hi + 1)), bool(rng.integers(0, 2))) for _ in range(k)]
        if k >= 5:
            b[2] = (0, True)
            b[3], b[4] = (b[3][0], True), (b[4][0], False)
        return b

    for hl in (0, 7, 19):
        for bc in (0, 1):
            for k in (0, 1, 5, 300):
                add("valid", "k=%d" % k, make_frame(rng, hl, some(k), bc), hl, bc, ST_OK, k)
            full = [(17, False), (WALK_BLOCK_SIZE, False), (WALK_BLOCK_SIZE, True), (3, True)]
            add("valid", "blocks of exactly block_size", make_frame(rng, hl, full, bc), hl, bc, ST_OK, 4)
            add("valid", "9 bytes behind the EndMark", make_frame(rng, hl, some(5), bc, behind=rng.integers(1, 256, 9, dtype=np.uint8).tobytes()),
                hl, bc, ST_OK, 5)
            more = make_frame(rng, 0, some(2), bc)                  # what lies behind the EndMark looks like two more blocks and an EndMark
            add("valid", "a frame's blocks behind the EndMark", make_frame(rng, hl, some(5), bc, behind=more), hl, bc, ST_OK, 5)
            add("valid", "max_blocks = k", make_frame(rng, hl, some(5), bc), hl, bc, ST_OK, 5, max_blocks=5)
            for stored in (False, True):
                for before in (0, 2):
                    b = some(before) + [(WALK_BLOCK_SIZE + 1, stored)] + some(1)
                    add("too_big", "block_size + 1 behind %d blocks, stored=%d" % (before, stored), make_frame(rng, hl, b, bc), hl, bc, ST_TOO_BIG, before)
            # (a too-big block that the frame does not hold in full is BlockTooBig all the same: the length is judged before the payload is read)
            f = make_frame(rng, hl, some(1) + [(0x7FFFFFFF, True, 11)], bc, endmark=False)
            add("too_big", "0x7FFFFFFF bytes announced at the end", f, hl, bc, ST_TOO_BIG, 1)
            f = make_frame(rng, hl, some(4) + [(int(rng.integers(20, 41)), False)], bc)
            for cut in range(1, 17):                                # 1..4: inside the EndMark; from 5 on: inside the last block
                add("cut", "%d bytes short" % cut, f, hl, bc, ST_TRUNCATED, 5 if cut <= 4 else 4, frame_len=len(f) - cut)
            f = make_frame(rng, hl, [(30, False), (25, True), (40, False), (12, True), (9, False)], bc)
            inside = hl + (4 + 30 + 4 * bc) + (4 + 25 + 4 * bc) + 4 + 20
            add("cut", "inside the third payload", f, hl, bc, ST_TRUNCATED, 2, frame_len=inside)
            add("cut", "behind the third word", f, hl, bc, ST_TRUNCATED, 2, frame_len=inside - 20)
            add("cut", "inside the third word", f, hl, bc, ST_TRUNCATED, 2, frame_len=inside - 21)
            f = make_frame(rng, hl, some(5), bc, endmark=False)     # (the zeros behind frame_len would be an EndMark)
            add("no_endmark", "the frame ends behind its last block", f + bytes(8), hl, bc, ST_TRUNCATED, 5, frame_len=len(f))
            add("no_endmark", "no block and no EndMark", make_frame(rng, hl, [], bc, endmark=False) + bytes(8), hl, bc, ST_TRUNCATED, 0, frame_len=hl)
            f = make_frame(rng, hl, some(5), bc)
            add("short", "frame_len = header_len + 3", f, hl, bc, ST_TRUNCATED, 0, frame_len=hl + 3)
            if hl:
                add("short", "frame_len = header_len - 1", f, hl, bc, ST_TRUNCATED, 0, frame_len=hl - 1)
                add("short", "frame_len = 0", f, hl, bc, ST_TRUNCATED, 0, frame_len=0)
            f = make_frame(rng, hl, some(5), bc)
            add("max_blocks", "max_blocks = k - 1", f, hl, bc, ST_MAX_BLOCKS, 4, max_blocks=4)
            add("max_blocks", "max_blocks = 0", f, hl, bc, ST_MAX_BLOCKS, 0, max_blocks=0)
            add("max_blocks", "max_blocks = 0, no block", make_frame(rng, hl, [], bc), hl, bc, ST_OK, 0, max_blocks=0)
    return cases


WALK_GROUPS = ("valid", "too_big", "cut", "no_endmark", "short", "max_blocks")


def walk_device(lib, c, slots):
    """lz4flex_frame_walk_device with tables of `slots` canary entries (>= max_blocks) and info of 4 + PAD canary words; returns
    (rc, info, payload_off, len_word), each whole"""
    assert slots >= c["max_blocks"]
    d_frame = _dev(np.frombuffer(c["frame"] + bytes(16), np.uint8))
    d_info, d_off, d_word = _dev(np.full(4 + PAD, CANARY32, np.uint32)), _dev(np.full(slots, CANARY64, np.uint64)), _dev(np.full(slots, CANARY32, np.uint32))
    s = _stream(d_frame)
    rc = lib.lz4flex_frame_walk_device(_p(d_frame), c["frame_len"], c["header_len"], c["block_checksums"], c["block_size"], c["max_blocks"],
                                       _p(d_off), _p(d_word), _p(d_info), C.c_void_p(s.cuda_stream))
    s.synchronize()
    return rc, _host(d_info, np.uint32), _host(d_off, np.uint64), _host(d_word, np.uint32)


def walk_images(c, slots):
    """(status, info with its canaries -- words 2..3 None where the status is not 0 --, payload_off, len_word) as walk_device must return them"""
    k, st, end, offs, words = ref_walk(c["frame"], c["frame_len"], c["header_len"], c["block_checksums"], c["block_size"], c["max_blocks"])
    info = [k, st] + ([end & 0xFFFFFFFF, end >> 32] if st == ST_OK else [None, None]) + [CANARY32] * PAD
    off = np.full(slots, CANARY64, np.uint64)
    off[:k] = offs
    word = np.full(slots, CANARY32, np.uint32)
    word[:k] = words
    return st, info, off, word
