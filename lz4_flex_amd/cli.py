"""`lz4`-like command line over the frame API (reference lz4_bin/src/main.rs:34-166), block bytes from the GPU.

    python -m lz4_flex_amd.cli FILE            -> FILE.lz4          python -m lz4_flex_amd.cli FILE.lz4 -> FILE
    python -m lz4_flex_amd.cli [-d] [-o OUT]   (stdin -> stdout / OUT)
Options as the reference's: --clean (delete the original), -f/--force (overwrite), -d/--decompress, -o/--out.
Beyond the reference: --range OFF:LEN with a decompression writes just those bytes of the content (frame.FrameIndex.read: only the
blocks the range touches are decoded; Independent frames; the content checksum is not verified); --high [--depth N] with a compression
takes the deep-search encoder (block.set_compress_mode("high"), N candidates per position, default 16): smaller blocks, more encode time;
--high --optimal parses its matches by price instead of lazily (block.set_compress_parse("optimal")): smaller again;
--linked with a compression writes a Linked frame (BlockMode.Linked: a block's matches reach into the blocks in front of it), and --high
--linked searches that history as deeply as the block (block.set_compress_high_linked(True)).
"""
import argparse
import os
import sys

from . import block
from .frame import BlockMode, FrameDecoder, FrameEncoder, FrameIndex, FrameInfo

LZ_EXTENSION = ".lz4"
CHUNK = 4 << 20


class _TrackWriteSize:   # main.rs:166-190
    def __init__(self, inner):
        self.inner, self.written = inner, 0

    def write(self, b):
        self.inner.write(b)
        self.written += len(b)
        return len(b)


def _copy(src, dst):     # io::copy
    n = 0
    while True:
        b = src.read(CHUNK)
        if not b:
            return n
        dst.write(b)
        n += len(b)


def _parse_range(text):
    try:
        off, _, length = text.partition(":")
        off, length = int(off, 0), int(length, 0)
    except ValueError:
        raise SystemExit("--range wants OFF:LEN, two non-negative integers")
    if off < 0 or length < 0:
        raise SystemExit("--range wants OFF:LEN, two non-negative integers")
    return off, length


def _decode(fin, fout, byte_range):
    if byte_range is None:
        _copy(FrameDecoder.new(fin), fout)
    else:
        with FrameIndex(fin.read()) as index:
            fout.write(index.read(*byte_range))


def _encoder(wtr, linked):
    return FrameEncoder.with_frame_info(FrameInfo(block_mode=BlockMode.Linked), wtr) if linked else FrameEncoder.new(wtr)


def handle_file(path, out, clean, force, force_decompress, print_info=True, byte_range=None, linked=False):   # main.rs:82-164
    decompress = path.endswith(LZ_EXTENSION)
    if force_decompress and not decompress:
        raise SystemExit("Can't determine an output filename")
    if out is None:
        out = path[:-len(LZ_EXTENSION)] if decompress else path + LZ_EXTENSION
        if print_info:
            print("%s filename will be: %s" % ("Decompressed" if decompress else "Compressed", out))
        if not force and os.path.exists(out):
            sys.stdout.write("%s already exists, do you want to overwrite? (y/N) " % out)
            sys.stdout.flush()
            if not sys.stdin.readline().startswith("y"):
                print("Not overwriting")
                return
    if decompress:
        with open(path, "rb") as fin, open(out, "wb") as fout:
            _decode(fin, fout, byte_range)
    else:
        with open(path, "rb") as fin, open(out, "wb") as fout:
            tw = _TrackWriteSize(fout)
            enc = _encoder(tw, linked)
            n_in = _copy(fin, enc)
            enc.finish()
            if print_info:
                print("Compressed %d bytes into %d ==> %.2f%%" % (n_in, tw.written, tw.written * 100.0 / max(n_in, 1)))
    if clean:
        os.remove(path)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="lz4_flex_amd.cli", description="[De]Compress data in the lz4 format.")
    ap.add_argument("--clean", action="store_true", help="delete original files (default: false)")
    ap.add_argument("-f", "--force", action="store_true", help="overwrite output files")
    ap.add_argument("-d", "--decompress", action="store_true", help="force decompress")
    ap.add_argument("input_file", nargs="?", help="file to compress/decompress ('-' or absent: stdin)")
    ap.add_argument("-o", "--out", help="output file to write to. defaults to stdout")
    ap.add_argument("--range", metavar="OFF:LEN", help="decompression: write only bytes [OFF, OFF + LEN) of the content")
    ap.add_argument("--high", action="store_true", help="compression: the deep-search encoder (smaller output, slower)")
    ap.add_argument("--depth", type=int, metavar="N", help="with --high: candidates examined per position, 1 .. 256 (default 16)")
    ap.add_argument("--optimal", action="store_true", help="with --high: the optimal parse (smaller output again, slower)")
    ap.add_argument("--linked", action="store_true", help="compression: a Linked frame (blocks may refer to the blocks in front of them)")
    o = ap.parse_args(argv)
    byte_range = _parse_range(o.range) if o.range else None
    if o.depth is not None and not o.high:
        raise SystemExit("--depth goes with --high")
    if o.depth is not None and not 1 <= o.depth <= 256:
        raise SystemExit("--depth wants 1 .. 256")
    if o.optimal and not o.high:
        raise SystemExit("--optimal goes with --high")
    if o.high:
        if o.decompress or (o.input_file and o.input_file.endswith(LZ_EXTENSION)):
            raise SystemExit("--high goes with a compression")
        block.set_compress_mode("high")
        if o.depth is not None:
            block.set_compress_depth(o.depth)
        if o.optimal:
            block.set_compress_parse("optimal")
        block.set_compress_high_linked(o.linked)
    if o.linked and (o.decompress or (o.input_file and o.input_file.endswith(LZ_EXTENSION))):
        raise SystemExit("--linked goes with a compression")
    if o.input_file and o.input_file != "-":
        if byte_range is not None and not o.input_file.endswith(LZ_EXTENSION):
            raise SystemExit("--range goes with a decompression")
        handle_file(o.input_file, o.out, o.clean, o.force, o.decompress, byte_range=byte_range, linked=o.linked)
        return 0
    if byte_range is not None and not o.decompress:
        raise SystemExit("--range goes with a decompression")
    fin = sys.stdin.buffer
    fout = open(o.out, "wb") if o.out else sys.stdout.buffer
    try:
        if o.decompress:
            _decode(fin, fout, byte_range)
        else:
            enc = _encoder(fout, o.linked)
            _copy(fin, enc)
            enc.finish()
    finally:
        if o.out:
            fout.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
