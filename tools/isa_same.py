#!/usr/bin/env python3
"""Is the device code of this tree's kernel sources the same as another checkout's?  For a refactor that must not change a kernel:
both trees' lz4_flex_amd.build.file_isa listings (`hipcc -S`, the build's flags) of a source file are compared line by line, whole
files, after dropping the lines that hold the per-compilation `__hip_cuid_` symbol.  No GPU needed.

    tools/isa_same.py PARENT_CHECKOUT [FILE [-DFLAG ...]] ...

Flags behind a file name belong to that file; a file may be given more than once.  Without files: every csrc/*.hip of this tree,
and again lz4_decompress_plan.hip and lz4_decompress_fused.hip with -DLZ4FLEX_TOOLS, lz4_compress.hip and lz4_decompress.hip with
-DLZ4FLEX_ALL_VARIANTS (code the default build leaves out).  One line per file: same / DIFFERENT, the listing's line count and
the source's line count in both trees.  Exit status 1 when a listing differs or a file does not compile."""
import concurrent.futures
import glob
import importlib.util
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORE = [("lz4_decompress_plan.hip", ["-DLZ4FLEX_TOOLS"]), ("lz4_decompress_fused.hip", ["-DLZ4FLEX_TOOLS"]),
        ("lz4_compress.hip", ["-DLZ4FLEX_ALL_VARIANTS"]), ("lz4_decompress.hip", ["-DLZ4FLEX_ALL_VARIANTS"])]


def build_module(root, name):
    """build.py of the checkout at `root`, loaded by path (the package itself would look for its library)"""
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "lz4_flex_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def n_lines(path):
    try:
        with open(path, "rb") as f:
            return sum(1 for _ in f)
    except OSError:
        return 0


def main(argv):
    if len(argv) < 2:
        print(__doc__, file=sys.stderr)
        return 2
    old, new = build_module(os.path.abspath(argv[1]), "isa_same_parent"), build_module(ROOT, "isa_same_tree")
    items = []
    for a in argv[2:]:
        if a.startswith("-"):
            items[-1][1].append(a)
        else:
            items.append((a, []))
    if not items:
        items = [(os.path.basename(p), []) for p in sorted(glob.glob(os.path.join(new.CSRC, "*.hip")))] + MORE
    locks = {src: threading.Lock() for src, _ in items}      # file_isa writes build/<file>_check.s: one compilation of a file at a time

    def one(item):
        src, flags = item
        with locks[src]:
            try:
                a, b = ([ln for ln in m.file_isa(src, flags) if "__hip_cuid_" not in ln] for m in (old, new))
            except (RuntimeError, OSError) as e:
                return False, "%-28s %-24s FAILED: %s" % (src, " ".join(flags), e)
        return a == b, "%-28s %-24s %-9s listing %6d -> %6d lines, source %5d -> %5d lines" % (
            src, " ".join(flags), "same" if a == b else "DIFFERENT", len(a), len(b), n_lines(os.path.join(old.CSRC, src)), n_lines(os.path.join(new.CSRC, src)))

    ok = True
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        for same, line in pool.map(one, items):
            print(line, flush=True)
            ok = ok and same
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
