"""An LZ4 block written sequence by sequence, with the plain text the format's byte-wise semantics give.  Test infrastructure
(a plain module, not a fixture): the GPU tests build blocks that sit on a kernel's boundaries with it, and the CPU tests check
that it and the oracle agree on what every such block says."""
import random


class Writer:
    """an LZ4 block, sequence by sequence (src/block/compress.rs:463-487 is the layout), with the plain text the format's byte-wise
    semantics give (decompress_safe.rs:93-247).  `prefix`: bytes that lie in the sink before the block (a Linked frame's earlier
    blocks, lz4flex_decompress_batch_ex's out_pos): offsets may reach into them, and end() returns only the block's own bytes."""

    def __init__(self, seed=1, prefix=b""):
        self.comp, self.rnd = bytearray(), random.Random(seed)
        self.out = bytearray(prefix)
        self.base = len(prefix)

    def _len(self, v):
        while v >= 255:
            self.comp.append(255)
            v -= 255
        self.comp.append(v)

    def _lits(self, lit):
        return bytes(self.rnd.getrandbits(8) for _ in range(lit)) if isinstance(lit, int) else bytes(lit)

    def _head(self, lits, off, ml):
        self.comp.append((min(len(lits), 15) << 4) | min(ml - 4, 15))
        if len(lits) >= 15:
            self._len(len(lits) - 15)
        self.comp += lits
        self.out += lits
        self.comp += bytes((off & 0xFF, off >> 8))
        if ml - 4 >= 15:
            self._len(ml - 19)

    def seq(self, lit, off, ml):
        lits = self._lits(lit)
        assert 1 <= off <= len(self.out) + len(lits) and off <= 65535 and ml >= 4, (off, len(self.out) + len(lits), ml)
        self._head(lits, off, ml)
        start = len(self.out) - off
        if off >= ml:
            self.out += self.out[start:start + ml]
        else:                                    # the source overlaps the destination: the byte-serial copy repeats the period
            pat = bytes(self.out[start:])
            self.out += (pat * (ml // off + 1))[:ml]
        return self

    def bad_seq(self, lit, off, ml):
        """a sequence whose offset the writer does not check (off > what lies behind it is OffsetOutOfBounds); the block's plain text
        is then the oracle's to say"""
        self._head(self._lits(lit), off, ml)
        return self

    def end(self, lit=5):
        lits = self._lits(lit)
        self.comp.append(min(lit, 15) << 4)
        if lit >= 15:
            self._len(lit - 15)
        self.comp += lits
        self.out += lits
        return bytes(self.comp), bytes(self.out[self.base:])
