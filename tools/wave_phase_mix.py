#!/usr/bin/env python3
"""Static instruction budget of the wave encoder (lz4_flex_amd/csrc/lz4_compress_wave.hip) per phase of the worker's superstep and per
step of the indexer: the listing of a -DLZ4W_MARK build (its "; LZ4W_PHASE_END i" markers are the LZ4W_TICK points of match_segment).

The superstep loop of match_segment (the blocks annotated with its header) is walked breadth-first from the header in phase 0; an
instruction belongs to the phase the walk is in when it first reaches the instruction's block, and a marker "PHASE_END i" moves the walk
to phase i + 1.  Phase 5 is what follows the merge: encode_seqs, inlined, and the loop latch.  Counts are static (every path of the
listing once: the NS = 4 and NS = 2 supersteps, the <= 64 and 65..128 head paths, every length round), a proxy for where the issue
slots go, not a dynamic count.  The indexer: the largest loop of index_window (four chunks of 16 steps) and that divided by 64.

usage: wave_phase_mix.py [--src FILE.hip] [--listing FILE.s] [--json]    (default: the tree's encoder, compiled here with hipcc)"""
import argparse
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "lz4_flex_amd", "csrc", "lz4_compress_wave.hip")
PHASES = ["heads", "compaction + lengths", "scan", "walk", "merge", "encode_seqs + latch"]
KINDS = ["valu", "salu", "lds", "vmem", "branch", "waitcnt", "other"]


def kind(op):
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    if op.startswith("s_cbranch") or op == "s_branch":
        return "branch"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "scratch_", "buffer_", "flat_")):
        return "vmem"
    return "other"


def compile_listing(src):
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    out = os.path.join(tempfile.mkdtemp(prefix="wave_phase_mix_"), "wave_mark.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-DLZ4W_MARK", "-x", "hip", "--cuda-device-only", "-S",
                           src, "-o", out], stderr=subprocess.DEVNULL)
    return open(out).read().split("\n")


def function(lines, name_part):
    """the lines of the first function whose mangled name contains name_part"""
    start = None
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m and start is None and name_part in m.group(1):
            start = i
        elif start is not None and (l.startswith(".Lfunc_end") or m):
            return lines[start:i]
    raise SystemExit("function %s not found" % name_part)


def blocks(fn):
    """[(label, annotation text, [instruction lines])] in layout order"""
    out = []
    cur = ["entry", "", []]
    for l in fn[1:]:
        m = re.match(r"^\.L(BB\d+_\d+):(.*)$", l)
        if m:
            out.append(cur)
            cur = [m.group(1), m.group(2), []]
            continue
        if l.startswith("; %bb."):            # a block without a label (fall-through only)
            out.append(cur)
            cur = [l.split(":")[0][2:], l, []]
            continue
        t = l.strip()
        if not t:
            continue
        if t.startswith(";") and not cur[2]:
            cur[1] += " " + t                  # the loop annotation of the block
        if l.startswith("\t"):
            cur[2].append(t)
    out.append(cur)
    return out


def superstep_budget(fn):
    bl = blocks(fn)
    hdr = None
    for lab, ann, _ in bl:
        if "Loop Header: Depth=1" in ann:
            hdr = lab
            break
    index = {lab: i for i, (lab, _, _) in enumerate(bl)}
    inloop = [lab == hdr or ("Header=%s " % hdr) in ann + " " or ("Parent Loop %s " % hdr) in ann + " " for lab, ann, _ in bl]
    counts = [collections.Counter() for _ in PHASES]
    seen = set()
    queue = collections.deque([(index[hdr], 0)])
    while queue:
        i, ph = queue.popleft()
        if i in seen or i >= len(bl) or not inloop[i]:
            continue
        seen.add(i)
        falls = True
        for t in bl[i][2]:
            m = re.match(r"; LZ4W_PHASE_END (\d+)", t)
            if m:
                ph = min(int(m.group(1)) + 1, len(PHASES) - 1)
                continue
            if t.startswith((";", ".")) or re.match(r"^\d+:", t):
                continue
            op = t.split()[0]
            counts[ph][kind(op)] += 1
            m = re.match(r"s_(?:cbranch_\w+|branch)\s+\.L(BB\d+_\d+)", t)
            if m and m.group(1) in index:
                queue.append((index[m.group(1)], ph))
            if op == "s_branch" and m:
                falls = False
        if falls:
            queue.append((i + 1, ph))
    return counts


def indexer_budget(fn):
    """the largest loop of index_window: {kind: count}"""
    loops = collections.OrderedDict()
    cur = None
    for l in fn:
        m = re.search(r"(?:in Loop: Header=|Parent Loop )(BB\d+_\d+)", l)
        h = re.match(r"^\.L(BB\d+_\d+):.*Loop Header", l)
        if l.startswith(".L") or l.startswith("; %bb"):
            cur = h.group(1) if h else (m.group(1) if m else None)
            continue
        if cur is None and m and not l.startswith("\t"):
            cur = m.group(1)
            continue
        if cur and l.startswith("\t"):
            t = l.strip()
            if t.startswith((";", ".")):
                continue
            loops.setdefault(cur, collections.Counter())[kind(t.split()[0])] += 1
    return max(loops.values(), key=lambda c: sum(c.values()))


def resources(lines, kernel_part="lz4_compress_wave_kernel"):
    txt = "\n".join(lines)
    m = re.search(r"\.name:\s+\S*%s\S*(.*?)\.vgpr_count:\s+(\d+)" % kernel_part, txt, re.S)
    vg = int(m.group(2)) if m else None
    m2 = re.search(r"\.name:\s+\S*%s\S*(.*?)\.private_segment_fixed_size:\s+(\d+)" % kernel_part, txt, re.S)
    sc = int(m2.group(2)) if m2 else None
    return vg, sc


def budget(lines):
    ms = function(lines, "match_segment")
    ss = superstep_budget(ms)
    ix = indexer_budget(function(lines, "index_window"))
    eg = collections.Counter(kind(l.strip().split()[0]) for l in function(lines, "emit_generic")
                             if l.startswith("\t") and not l.strip().startswith((";", ".")))
    scratch = sum(1 for l in ms if re.match(r"\s+scratch_(load|store)", l))
    vg, priv = resources(lines)
    return {"phases": {PHASES[i]: dict(ss[i]) for i in range(len(PHASES))},
            "superstep_total": dict(sum(ss, collections.Counter())),
            "indexer_4_chunks": dict(ix), "indexer_per_step": {k: round(v / 64.0, 2) for k, v in ix.items()},
            "emit_generic": dict(eg), "match_segment_scratch_ops": scratch, "vgpr_count": vg, "private_segment_bytes": priv}


def table(b):
    rows = [("phase",) + tuple(KINDS) + ("total",)]
    for name, c in list(b["phases"].items()) + [("superstep loop", b["superstep_total"]), ("indexer, 4 chunks", b["indexer_4_chunks"]),
                                                 ("emit_generic (a call)", b["emit_generic"])]:
        rows.append((name,) + tuple(str(c.get(k, 0)) for k in KINDS) + (str(sum(c.values())),))
    w = [max(len(r[i]) for r in rows) for i in range(len(rows[0]))]
    s = "\n".join("  ".join(r[i].rjust(w[i]) if i else r[i].ljust(w[i]) for i in range(len(r))) for r in rows)
    s += "\nindexer per 64-position step: %s" % b["indexer_per_step"]
    s += "\nkernel: %s VGPRs, %s B private segment; match_segment: %d scratch operations" % (
        b["vgpr_count"], b["private_segment_bytes"], b["match_segment_scratch_ops"])
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=SRC)
    ap.add_argument("--listing", default=None, help="a listing made with -DLZ4W_MARK (else --src is compiled)")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    lines = open(a.listing).read().split("\n") if a.listing else compile_listing(a.src)
    b = budget(lines)
    print(json.dumps(b, indent=1) if a.json else table(b))


if __name__ == "__main__":
    sys.exit(main())
