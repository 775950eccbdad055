#!/usr/bin/env python3
"""Do two `hipcc -S` listings of lz4_compress_wave.hip (or of another kernel file of a namespace of lz4flex_dev, such as
lz4_compress_high.hip with the function lz4_compress_high_kernel) hold the same instruction streams for the hot functions?

    python tools/isa_fn_diff.py PARENT.s CHANGE.s [function ...]        (default: match_segment index_window)

A listing is what lz4_flex_amd.build.wave_isa() leaves in lz4_flex_amd/build/lz4_compress_wave_check.s (the build's flags,
--cuda-device-only -S).  Per function: instructions only -- comments, directives and the numbering of local labels are dropped --
then a unified diff.  Exit status 1 when any function differs."""
import difflib
import re
import sys


def functions(path, names):
    with open(path) as f:
        text = f.read()
    out = {}
    pat = r"^(_ZN11lz4flex_dev\d+[a-z]+\d+(?:%s)\w*):.*?^\.Lfunc_end\d+:" % "|".join(names)
    for m in re.finditer(pat, text, re.S | re.M):
        body = []
        for line in m.group(0).splitlines()[1:-1]:
            code = line.split(";")[0].strip()
            if not code or code.startswith("."):
                continue
            body.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", code))
        info = re.search(re.escape(m.group(1)) + r": ; @.*?; NumVgprs: (\d+).*?; ScratchSize: (\d+)", text, re.S)
        out[m.group(1)] = (body, info.groups() if info else ("?", "?"))
    return out


def main():
    names = sys.argv[3:] or ["match_segment", "index_window"]
    a, b = functions(sys.argv[1], names), functions(sys.argv[2], names)
    differ = False
    for k in sorted(set(a) | set(b)):
        (ia, ra), (ib, rb) = a.get(k, ([], ("-", "-"))), b.get(k, ([], ("-", "-")))      # ("-": the listing has no such function)
        d = list(difflib.unified_diff(ia, ib, lineterm="", n=0))
        print("%s: %d / %d instructions, VGPRs %s / %s, scratch %s / %s, %d diff lines" % (k[:64], len(ia), len(ib), ra[0], rb[0], ra[1], rb[1], len(d)))
        for line in d[:40]:
            print("    " + line)
        differ |= bool(d) or ra != rb
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
